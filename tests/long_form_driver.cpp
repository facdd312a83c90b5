// Test infrastructure: drives the splitter of long-form text (rule C15s; tokenizer.cpp, no HIP) so that the CPU suite can compare it with
// tests/long_form_ref.py and run it under the host sanitizers.  usage: driver <model.bin> <cases.bin>
// cases.bin: repeated records { int32 max_tokens; int32 n_bytes; n_bytes of text }.  Prints one line per record: the spans as "begin end" pairs,
// or "error" where the splitter refuses (max_tokens outside 0 .. 255, more than 64 chunks).
#include "model_file.h"
#include "tokenizer.h"

#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <stdexcept>
#include <string>
#include <vector>

int main(int argc, char ** argv) {
    if (argc != 3) return 2;
    barkhip::ModelFile mf;
    std::string err;
    if (!mf.open(argv[1], err)) { fprintf(stderr, "%s\n", err.c_str()); return 1; }
    barkhip::Vocab vocab;
    vocab.build(mf.vocab);
    std::ifstream in(argv[2], std::ios::binary);
    const std::string raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    for (size_t pos = 0; pos + 8 <= raw.size();) {
        int32_t max_tokens, n;
        memcpy(&max_tokens, raw.data() + pos, 4);
        memcpy(&n, raw.data() + pos + 4, 4);
        pos += 8;
        if (n < 0 || pos + (size_t) n > raw.size()) { fprintf(stderr, "truncated case file\n"); return 1; }
        const std::string text = raw.substr(pos, (size_t) n);
        pos += (size_t) n;
        try {
            const std::vector<barkhip::TextSpan> spans = barkhip::split_text(vocab, text, max_tokens);
            for (const barkhip::TextSpan & s : spans) printf("%d %d ", s.begin, s.end);
            printf("\n");
        } catch (const std::runtime_error &) { printf("error\n"); }
    }
    return 0;
}
