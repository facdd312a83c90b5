// Drives the number parsing of bark.cpp_amd/examples/http_util.h on the CPU: argv[1] = a JSON body; prints "top_k=<status>,<value>" and
// "top_p=<status>,<value as %a>" - status 0: absent, 1: parsed, -1: malformed (the server answers 400).
#include "http_util.h"

#include <cstdio>

int main(int argc, char ** argv) {
    const std::string body = argc > 1 ? argv[1] : "";
    int32_t k = 0; float p = 1.0f;
    const int rk = barkhttp::json_int(body, "top_k", k);
    const int rp = barkhttp::json_float(body, "top_p", p);
    printf("top_k=%d,%d\n", rk, (int) k);
    printf("top_p=%d,%a\n", rp, (double) p);
    return 0;
}
