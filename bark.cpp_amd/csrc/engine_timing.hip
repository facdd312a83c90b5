// engine_timing.hip - hipEvent-timed replays of single kernels / decode steps / fine passes for bench.py's roofline block.
#include "engine_internal.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <stdexcept>

using namespace barkhip;
using namespace barkhip::detail;

namespace barkhip {

// ---------------------------------------------------------------------------------------------------
// timing hooks for bench.py (hipEvents on the engine's own stream)
// ---------------------------------------------------------------------------------------------------
// ONE top-k / nucleus filter launch over n_slots rows of n logits (C8n's kernel alone).  The filter masks its rows in place, so every launch gets the
// original rows back first (a device copy outside the timed interval).  peaked: N(0, 1) logits times 4 (a nucleus of a few hundred ids at n = 10 048);
// flat: N(0, 1) logits times 0.01 (nucleus ~ n).
double engine_time_sample_filtered(bark_context * c, int n, int n_slots, int top_k, float top_p, int peaked, int iters) {
    if (n < 1 || n > 12288 || n_slots < 1 || n_slots > 256 || !filter_valid(bark_hip_sampling_filter{top_k, top_p})) throw std::runtime_error("time_sample_filter: bad arguments");
    HIP_OK(hipSetDevice(c->device));
    std::mt19937 g(1234);
    std::normal_distribution<float> nd(0.0f, 1.0f);
    std::vector<float> rows((size_t) n_slots * n);
    for (auto & v : rows) v = nd(g) * (peaked ? 4.0f : 0.01f);
    struct Buf { void * p = nullptr; ~Buf() { if (p) (void) hipFree(p); } } orig, work, par;
    HIP_OK(hipMalloc(&orig.p, rows.size() * 4)); HIP_OK(hipMalloc(&work.p, rows.size() * 4)); HIP_OK(hipMalloc(&par.p, (size_t) n_slots * 8));
    std::vector<int32_t> pk((size_t) n_slots, top_k); std::vector<float> pp((size_t) n_slots, top_p);
    HIP_OK(hipMemcpyAsync(orig.p, rows.data(), rows.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipMemcpyAsync(par.p, pk.data(), (size_t) n_slots * 4, hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipMemcpyAsync((char *) par.p + (size_t) n_slots * 4, pp.data(), (size_t) n_slots * 4, hipMemcpyHostToDevice, c->stream));
    FilterArgs f;
    f.logits = (float *) work.p; f.n = n; f.ld_logits = n; f.nbatch = n_slots; f.temp = 1.0f;
    f.top_k = (const int32_t *) par.p; f.top_p = (const float *) ((char *) par.p + (size_t) n_slots * 4);
    double total_us = 0.0;
    iters = std::max(1, iters);
    for (int i = -2; i < iters; i++) {                                    // two warm-up launches
        HIP_OK(hipMemcpyAsync(work.p, orig.p, rows.size() * 4, hipMemcpyDeviceToDevice, c->stream));
        const double us = time_on_stream_us(c, [&] { launch_sample_filter(c->stream, f); });
        if (i >= 0) total_us += us;
    }
    return total_us / iters;
}

double engine_time_decode_step(bark_context * c, int which, int ctxlen, int iters, double * bytes_per_step) {
    if (which < 0 || which > 1) throw std::runtime_error("time_decode_step: which must be 0 or 1");
    HIP_OK(hipSetDevice(c->device));
    GptModel & m = c->gpt[which];
    GptRun & run = c->gpt_run[which];
    ctxlen = std::max(1, std::min(ctxlen, m.hp.block_size));
    const StageCfg s = stage_cfg(c, which);
    StepState st = fresh_state(); st.n_past = ctxlen - 1; st.cur_token = 1;
    set_state(c, st);
    // the cache rows below ctxlen hold whatever the last run left; timing does not depend on the values,
    // but keep them finite: zero them once
    HIP_OK(hipMemsetAsync(run.kcache, 0, m.kv_layer_stride * m.hp.n_layer * 4, c->stream));
    HIP_OK(hipMemsetAsync(run.vcache, 0, m.kv_layer_stride * m.hp.n_layer * 4, c->stream));
    if (run.vtcache) HIP_OK(hipMemsetAsync(run.vtcache, 0, m.kv_layer_stride * m.hp.n_layer * 4, c->stream));
    // the graph the stage loops replay: eight steps per launch; n_past does not advance here
    const int per_graph = 8;
    upload_filter(c);                                                     // the step samples with the context's top-k / nucleus filter, if any
    run.bench_graph.reset();                                              // the variant depends on the context length
    run.bench_graph = capture_decode(c, s, 0, per_graph, (ctxlen + 255) / 256);
    for (int i = 0; i < 3; i++) HIP_OK(hipGraphLaunch(run.bench_graph.get(), c->stream));
    set_state(c, st);
    iters = std::max(1, iters / per_graph) * per_graph;
    const double us = time_on_stream_us(c, [&] {
        for (int i = 0; i < iters; i += per_graph) {
            HIP_OK(hipGraphLaunch(run.bench_graph.get(), c->stream));
            if (((i / per_graph) & 127) == 127) set_state(c, st);         // out_tokens holds 2048 entries
        }
    });
    if (bytes_per_step) {
        const double E = m.hp.n_embd, L = m.hp.n_layer;
        // f16 weights of all layers + evaluated LM-head rows + f32 K and V rows read
        const double wb = weight_bytes_per_element(m);
        *bytes_per_step = L * 12.0 * E * E * wb + (double) s.lm_rows * E * wb + 2.0 * ctxlen * E * L * 4.0;
    }
    return us / std::max(1, iters);
}

// One decode GEMV, launched `iters` times back to back while rotating through the layers' weights (so that the
// stream comes from HBM / Infinity Cache like in a real step, not from a hot L2).  op: 0 LN+QKV, 1 proj,
// 2 LN+FC+GELU, 3 mlp proj.  Returns the average device time per launch in microseconds.
double engine_time_gemv(bark_context * c, int which, int op, int iters, double * bytes_per_launch) {
    if (which < 0 || which > 1 || op < 0 || op > 7) throw std::runtime_error("time_gemv: bad arguments");
    const bool hot = op >= 4;
    op &= 3;
    HIP_OK(hipSetDevice(c->device));
    GptModel & m = c->gpt[which];
    const int E = m.hp.n_embd;
    StepState st = fresh_state(); st.n_past = 100; st.cur_token = 1;
    set_state(c, st);
    HIP_OK(hipMemsetAsync(c->x, 0, (size_t) E * 4, c->stream));
    HIP_OK(hipMemsetAsync(c->att, 0, (size_t) E * 2, c->stream));
    HIP_OK(hipMemsetAsync(c->hbuf, 0, (size_t) 4 * E * 2, c->stream));
    if (m.q4) { HIP_OK(hipMemsetAsync(c->att32, 0, (size_t) E * 4, c->stream)); HIP_OK(hipMemsetAsync(c->h32, 0, (size_t) 4 * E * 4, c->stream)); }
    auto launch = [&](int l) {
        LinArgs a = layer_product(c, m, l, op);
        a.N = 1;
        switch (op) {
            case OP_QKV:  a.x_f32 = c->x; a.q = c->q; a.kc = layer_k(c, m, l); a.vc = layer_v(c, m, l); a.st = c->d_state; break;
            case OP_PROJ: if (m.q4) a.x_f32 = c->att32; else a.x_f16 = c->att; a.res = c->x; break;
            case OP_FC:   a.x_f32 = c->x; a.out_h = c->hbuf; a.out_h32 = m.q4 ? c->h32 : nullptr; break;
            default:      if (m.q4) a.x_f32 = c->h32; else a.x_f16 = c->hbuf; a.res = c->x; break;
        }
        launch_linear(c->stream, a);
    };
    // op >= 4 ("hot"): always layer 0, so the weights stay in L2; otherwise rotate through the layers.
    // The launches are captured into one hipGraph (48 nodes) so that the host launch rate does not bound the result.
    const int per_graph = 48;
    const GraphExec exec = capture_graph(c->stream, [&] { for (int i = 0; i < per_graph; i++) launch(hot ? 0 : i % m.hp.n_layer); });
    HIP_OK(hipGraphLaunch(exec.get(), c->stream));
    const int reps = std::max(1, iters / per_graph);
    const double us = time_on_stream_us(c, [&] { for (int i = 0; i < reps; i++) HIP_OK(hipGraphLaunch(exec.get(), c->stream)); });
    iters = reps * per_graph;
    if (bytes_per_launch) {
        const double Ed = E;
        const double w = op == 0 ? 3 * Ed * Ed : op == 1 ? Ed * Ed : 4 * Ed * Ed;
        *bytes_per_launch = w * weight_bytes_per_element(m);          // the weight matrix; vectors are < 1 % of it
    }
    return us / std::max(1, iters);
}

#ifdef BARK_TRACE
// diagnostic build: `replays` consecutive replays of one decode step with per-wave time stamps; returns the record count
int engine_trace_decode_step(bark_context * c, int which, int ctxlen, int replays, unsigned long long * out6, int cap_records) {
    HIP_OK(hipSetDevice(c->device));
    GptModel & m = c->gpt[which];
    GptRun & run = c->gpt_run[which];
    const StageCfg s = stage_cfg(c, which);
    StepState st = fresh_state(); st.n_past = ctxlen - 1; st.cur_token = 1;
    set_state(c, st);
    if (!c->trace_rec) {
        c->trace_cap = 1u << 19;
        c->trace_rec = dev_alloc<unsigned long long>(c, (size_t) c->trace_cap * 8);
        c->trace_pos = dev_alloc<unsigned>(c, 1);
    }
    HIP_OK(hipMemsetAsync(run.kcache, 0, m.kv_layer_stride * m.hp.n_layer * 4, c->stream));
    HIP_OK(hipMemsetAsync(run.vcache, 0, m.kv_layer_stride * m.hp.n_layer * 4, c->stream));
    if (run.vtcache) HIP_OK(hipMemsetAsync(run.vtcache, 0, m.kv_layer_stride * m.hp.n_layer * 4, c->stream));
    // first capture counts the waves of a step, the second bakes the per-replay stride into the kernels' arguments
    c->trace_kid = 0; c->trace_base = 0; c->trace_per_replay = 0;
    GraphExec g = capture_decode(c, s, 0, 1, (ctxlen + 255) / 256);
    g.reset();
    c->trace_per_replay = c->trace_base; c->trace_kid = 0; c->trace_base = 0;
    g = capture_decode(c, s, 0, 1, (ctxlen + 255) / 256);
    HIP_OK(hipMemsetAsync(c->trace_rec, 0, (size_t) c->trace_cap * 8 * sizeof(unsigned long long), c->stream));
    for (int i = 0; i < 5; i++) { HIP_OK(hipMemsetAsync(c->trace_pos, 0, sizeof(unsigned), c->stream)); HIP_OK(hipGraphLaunch(g.get(), c->stream)); }
    HIP_OK(hipStreamSynchronize(c->stream));
    set_state(c, st);
    HIP_OK(hipMemsetAsync(c->trace_pos, 0, sizeof(unsigned), c->stream));
    for (int i = 0; i < replays; i++) HIP_OK(hipGraphLaunch(g.get(), c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    unsigned n = c->trace_per_replay * (unsigned) replays;
    n = std::min(n, std::min(c->trace_cap, (unsigned) std::max(0, cap_records)));
    copy_to_host(c, out6, c->trace_rec, (size_t) n * 8 * sizeof(unsigned long long));
    return (int) n;
}
#endif

double engine_time_fine_pass(bark_context * c, int iters, double * flops_per_pass, int Z) {
    HIP_OK(hipSetDevice(c->device));
    GptModel & m = c->gpt[2];
    if (Z < 1 || Z > 32) throw std::runtime_error("time_fine_pass: 1..32 windows");
    std::vector<int32_t> buf((size_t) 8 * 1024 * Z);
    for (size_t i = 0; i < buf.size(); i++) buf[i] = (int32_t) ((i * 2654435761u) >> 22) & 1023;
    RowBufs rb = own_rows(c);
    if (Z > 1) {
        if (m.q4 || m.w32) throw std::runtime_error("time_fine_pass: several windows side by side need an f16 model file");
        ensure_fine_batch(c, Z);
        rb = fine_batch_rows(c, Z);
        HIP_OK(hipMemcpyAsync(c->fine_batch.tokens, buf.data(), buf.size() * 4, hipMemcpyHostToDevice, c->stream));
        HIP_OK(hipStreamSynchronize(c->stream));
    } else upload_tokens(c, buf.data(), buf.size());
    // Z > 1 is the pass of a lock-step job (engine_fine_many): C1m products under the default policy of bark_context::fine_order
    std::unique_ptr<JobScope> job;
    if (Z > 1) job.reset(new JobScope(c));
    auto pass = [&](int nn) { if (Z > 1) run_fine_forward(c, nn, 1024, &rb, Z); else run_fine_forward(c, nn, 1024); };
    pass(4);
    HIP_OK(hipStreamSynchronize(c->stream));
    const double us = time_on_stream_us(c, [&] { for (int i = 0; i < iters; i++) pass(2 + i % 6); });
    if (flops_per_pass) {
        const double E = m.hp.n_embd, L = m.hp.n_layer, N = 1024;
        *flops_per_pass = Z * (2.0 * N * (L * 12.0 * E * E + 1024.0 * E) + 4.0 * N * N * E * L);     // SURVEY.md 8(d), per window
    }
    return us / std::max(1, iters);
}

}  // namespace barkhip
