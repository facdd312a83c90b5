// output_format_driver.cpp - drives wav_samples / sample_format_of of bark.cpp_amd/examples/http_util.h without a device (tests/test_output_format_abi.py).
//   wav FORMAT RATE IN OUT     IN: raw samples in FORMAT ("f32" | "s16" | "mulaw"); OUT: the WAV wav_samples frames them in; prints "ok <samples> <bytes>"
// Exit status 0 whenever the helpers returned; anything else is a crash.
#include "http_util.h"

int main(int argc, char ** argv) {
    if (argc != 6 || std::string(argv[1]) != "wav") { fprintf(stderr, "usage: %s wav FORMAT RATE IN OUT\n", argv[0]); return 2; }
    const int format = barkhttp::sample_format_of(argv[2]);
    if (format < 0) { printf("err unknown format\n"); return 0; }
    std::string data;
    FILE * f = fopen(argv[4], "rb");
    if (!f) return 2;
    char buf[65536];
    for (size_t k; (k = fread(buf, 1, sizeof(buf), f)) > 0;) data.append(buf, k);
    fclose(f);
    const int width = format == 0 ? 4 : format == 1 ? 2 : 1;
    const int n = (int) (data.size() / (size_t) width);
    const std::string wav = barkhttp::wav_samples(data.data(), n, atoi(argv[3]), format);
    f = fopen(argv[5], "wb");
    if (!f) return 2;
    fwrite(wav.data(), 1, wav.size(), f);
    fclose(f);
    printf("ok %d %zu\n", n, wav.size());
    return 0;
}
