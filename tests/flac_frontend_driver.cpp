// flac_frontend_driver.cpp - drives the request parsing of bark_batch_server's output format without a device (tests/test_flac_frontend.py):
//   parse <json body> <default rate> <default format name>   prints "ok <rate> <format> <content type>" or "bad"
#include "http_util.h"

#include <cstdio>
#include <cstdlib>
#include <string>

int main(int argc, char ** argv) {
    if (argc == 5 && std::string(argv[1]) == "parse") {
        int32_t rate = atoi(argv[3]), format = barkhttp::sample_format_of(argv[4]);
        if (!barkhttp::request_format(argv[2], rate, format)) { printf("bad\n"); return 0; }
        printf("ok %d %d %s\n", rate, format, barkhttp::answer_type(format));
        return 0;
    }
    fprintf(stderr, "usage: %s parse <json> <rate> <format>\n", argv[0]);
    return 2;
}
