// resource_driver.cpp - walks one context of the host-emulated engine (tests/simt) through every way it acquires and releases graphs, events, grown
// scratch and pinned memory, in a process of its own that is linked with AddressSanitizer (tests/test_resource_ownership_host.py builds and runs it):
//   resource_driver MODEL       MODEL: the toy model file
// A double release, a release of something still in use or a forgotten one is the sanitizer's report (and a non-zero exit status); a call whose result
// is not the expected one is exit status 1.  The fine stage is left out: minutes under emulation.
#include "bark.h"
#include "bark_mi355x.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "resource_driver: %s failed (line %d)\n", #cond, __LINE__); exit(1); } } while (0)

static std::vector<float> decode(bark_context * c, int T) {
    std::vector<int32_t> codes((size_t) 8 * T);
    for (size_t i = 0; i < codes.size(); i++) codes[i] = (int32_t) ((i * 7 + 3) % 1024);
    std::vector<float> pcm((size_t) 320 * T);
    CHECK(bark_hip_codec_decode(c, codes.data(), 8, T, pcm.data(), (int) pcm.size()) == 320 * T);
    return pcm;
}

static std::vector<int32_t> semantic(bark_context * c, const int32_t * prompt) {
    std::vector<int32_t> out(64);
    const int n = bark_hip_semantic(c, prompt, out.data(), (int) out.size(), nullptr);
    CHECK(n > 0);
    out.resize((size_t) n);
    return out;
}

int main(int argc, char ** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s MODEL\n", argv[0]); return 2; }
    bark_context_params params = bark_context_default_params();
    params.temp = 0.0f; params.fine_temp = 0.0f; params.n_steps_text_encoder = 12;
    bark_context * c = bark_load_model(argv[1], params, 0);
    CHECK(c);

    // codec decode: growth (3 -> 70 frames), recapture of the LSTM block and the conv stack, replay on the grown buffers (5)
    const std::vector<float> pcm5_first = (decode(c, 3), decode(c, 70), decode(c, 5));

    // 12 decode steps: the eight-step and the one-step graph; switching the filter on and off drops them, the stage captures them again
    int32_t prompt[513];
    CHECK(bark_hip_tokenize(c, "hello world this is bark", prompt) == 513);
    const std::vector<int32_t> sem = semantic(c, prompt);
    bark_hip_stats st{};
    bark_hip_get_stats(c, &st);
    CHECK(st.graph_replays > 0);
    CHECK(bark_hip_set_sampling_filter(c, 5, 0.9f) == 0);
    CHECK(semantic(c, prompt) == sem);                           // greedy: the filter does not take part
    CHECK(bark_hip_set_sampling_filter(c, 0, 1.0f) == 0);
    CHECK(semantic(c, prompt) == sem);

    // timing hooks: a graph of the call's own, and the context's bench_graph (twice: the second call replaces the first's)
    double bytes = 0.0;
    CHECK(bark_hip_time_gemv(c, 0, 0, 48, &bytes) >= 0.0);
    CHECK(bark_hip_time_decode_step(c, 0, 40, 8, &bytes) >= 0.0);
    CHECK(bark_hip_time_decode_step(c, 0, 300, 8, &bytes) >= 0.0);

    // pinned memory, the tail clone, the events of a profiled lock step and its captured form
    CHECK(bark_hip_reserve_batch(c, 2) == 0);
    std::vector<char> json(1 << 16);
    CHECK(bark_hip_profile_lock_step(c, 0, 2, 40, 1, json.data(), (int) json.size()) > 0);

    // a call that throws inside the engine, behind the scratch of the calls before it
    {
        std::vector<int32_t> codes((size_t) 8 * 4, 1);
        codes[5] = 1 << 20;
        std::vector<float> pcm((size_t) 320 * 4);
        CHECK(bark_hip_codec_decode(c, codes.data(), 8, 4, pcm.data(), (int) pcm.size()) < 0);
    }

    // a clone of a context that has replayed graphs captures its own, and outlives the original
    bark_context * k = bark_hip_clone_context(c, 1);
    CHECK(k);
    CHECK(decode(k, 5) == pcm5_first);
    bark_free(c);
    CHECK(semantic(k, prompt) == sem);
    CHECK(decode(k, 5) == pcm5_first);
    bark_free(k);
    printf("ok\n");
    return 0;
}
