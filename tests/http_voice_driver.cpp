// Drives the voice-prompt side of bark.cpp_amd/examples/http_util.h on the CPU: argv[1] = a JSON body, argv[2..] = --voice arguments (name=file).
// Prints "load=<ok|error text>" per argument, then "voice=<status>,<n_sem>,<Tc>,<Tf>,<checksum>" - status 0: the field is absent, 1: the named voice,
// -1: not a string or an unknown name (the server answers 400).
#include "http_util.h"

#include <cstdio>

int main(int argc, char ** argv) {
    const std::string body = argc > 1 ? argv[1] : "";
    std::map<std::string, barkhttp::VoiceFile> table;
    for (int i = 2; i < argc; i++) {
        std::string err;
        printf("load=%s\n", barkhttp::add_voice(table, argv[i], err) ? "ok" : err.c_str());
    }
    const barkhttp::VoiceFile * v = nullptr;
    const int r = barkhttp::request_voice(body, table, &v);
    long long sum = 0;
    if (v) { for (int32_t x : v->semantic) sum += x; for (int32_t x : v->coarse) sum += 3 * (long long) x; for (int32_t x : v->fine) sum += 7 * (long long) x; }
    printf("voice=%d,%zu,%zu,%zu,%lld\n", r, v ? v->semantic.size() : 0, v ? v->coarse.size() / 2 : 0, v ? v->fine.size() / 8 : 0, sum);
    return 0;
}
