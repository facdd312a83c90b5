// engine_internal.h - declarations shared by the engine's translation units (engine_load.hip: model upload, a context's runtime state and its
// release; engine.hip: building blocks and the stage loops; engine_batch.hip: lock-step batching; engine_codec.hip: EnCodec decode and encode,
// semantic encoder, resamplers; engine_timing.hip: bench hooks).  Every launch descriptor that follows from the model alone is stated once here /
// in engine.hip (layer_product, lm_head_args, set_token_embedding), and so are graph capture (capture_graph), event timing (time_on_stream_us)
// and the fine stage's window plan (fine_plan / fine_window / fine_write_back).  Who owns what: the owner types of
// engine.h (GraphExec, Event, DevBuf) and the two allocators of a context here (dev_alloc, host_alloc).  Not an API.
#pragma once
#include "engine.h"

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <functional>
#include <stdexcept>
#include <string>
#include <vector>

#define HIP_OK(expr)                                                                                         \
    do {                                                                                                     \
        hipError_t _e = (expr);                                                                              \
        if (_e != hipSuccess)                                                                                \
            throw std::runtime_error(std::string("HIP error: ") + hipGetErrorString(_e) + " at " #expr);   \
    } while (0)

// diagnostic build: hand the context's trace log to a kernel's argument block and number the launch
#ifdef BARK_TRACE
#define BARK_TRACE_SET(c, args, nwaves) do { (args).tr.rec = (c)->trace_rec; (args).tr.pos = (c)->trace_pos; (args).tr.cap = (c)->trace_cap; (args).tr.kid = (c)->trace_kid++; (args).tr.base = (c)->trace_base; (args).tr.per_replay = (c)->trace_per_replay; (c)->trace_base += (unsigned) (nwaves); } while (0)
#else
#define BARK_TRACE_SET(c, args, nwaves) do { } while (0)
#endif

namespace barkhip { namespace detail {

inline int64_t now_us() {
    return std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// BARK_HIP_POISON=1 (diagnostic): every run-time allocation (KV caches, slot rows, scratch, partial scores) starts as 0xFF bytes - NaN as
// f32 / f16, -1 as an id - so that a read of memory nobody has written shows up in the results whatever a fresh box happens to hand out
// (the GPU suite is expected to pass unchanged under it)
inline bool poison_allocations() {
    static const bool v = getenv("BARK_HIP_POISON") && atoi(getenv("BARK_HIP_POISON")) != 0;
    return v;
}
// BARK_HIP_GUARD=1 (diagnostic): every run-time allocation sits between two 64 KB guard bands filled with 0xA5; guard_check() (engine_load.hip)
// verifies them at the end of every lock-step job and when the context is freed - a write of any kernel of the process that lands just outside one of
// this context's buffers (or runs over from a neighbour) is reported on stderr with the buffer's index and the offset
constexpr size_t kGuardBytes = 64 * 1024;
inline bool guard_allocations() {
    static const bool v = getenv("BARK_HIP_GUARD") && atoi(getenv("BARK_HIP_GUARD")) != 0;
    return v;
}
template <typename T> T * dev_alloc(bark_context * ctx, size_t count) {
    void * p = nullptr;
    const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
    if (guard_allocations() && ctx->stream) {
        const size_t body = (bytes + 255) & ~(size_t) 255;
        HIP_OK(hipMalloc(&p, body + 2 * kGuardBytes));
        ctx->allocs.push_back(p);
        ctx->guarded.push_back({p, body});
        HIP_OK(hipMemsetAsync(p, 0xA5, body + 2 * kGuardBytes, ctx->stream));
        if (poison_allocations()) HIP_OK(hipMemsetAsync((char *) p + kGuardBytes, 0xFF, body, ctx->stream));
        HIP_OK(hipStreamSynchronize(ctx->stream));
        return (T *) ((char *) p + kGuardBytes);
    }
    HIP_OK(hipMalloc(&p, bytes));
    ctx->allocs.push_back(p);
    if (poison_allocations() && ctx->stream) {
        HIP_OK(hipMemsetAsync(p, 0xFF, bytes, ctx->stream));
        HIP_OK(hipStreamSynchronize(ctx->stream));
    }
    return (T *) p;
}
int guard_check(bark_context * ctx, const char * where);      // number of damaged guard bands (0 without BARK_HIP_GUARD)
// pinned host memory of the context (freed with it, behind the device allocations)
template <typename T> T * host_alloc(bark_context * ctx, size_t count) {
    void * p = nullptr;
    HIP_OK(hipHostMalloc(&p, std::max<size_t>(count, 1) * sizeof(T), hipHostMallocDefault));
    ctx->pinned.push_back(p);
    return (T *) p;
}
} }  // namespace barkhip::detail

template <typename T> void barkhip::DevBuf<T>::reserve(bark_context * ctx, size_t count) {
    if (count > n) { p = detail::dev_alloc<T>(ctx, count); n = count; }
}
inline void barkhip::Event::record(hipStream_t s) {
    if (!e) HIP_OK(hipEventCreate(&e));
    HIP_OK(hipEventRecord(e, s));
}

namespace barkhip { namespace detail {

// device -> host on the context's own (non-blocking) stream, complete on return: never the legacy stream, which refuses work while ANY blocking
// stream of the process captures a graph (other contexts on other host threads do)
inline void copy_to_host(bark_context * c, void * dst, const void * src, size_t bytes) {
    HIP_OK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
}

// rows [row0, ...) of a weight matrix behind a QMat handle (block formats or f32)
inline QMat q4_rows(const QMat & w, size_t row0, int K) {
    QMat r = w;
    if (w.qt == QT_F32) { r.qs = w.qs + row0 * (size_t) K * 4; return r; }
    const size_t nb = row0 * (size_t) (K / 32);
    r.d = w.d + nb; r.qs = w.qs + nb * (size_t) quant_formats()[w.qt].qs_bytes;
    if (w.m) r.m = w.m + nb;
    if (w.qh) r.qh = w.qh + nb;
    return r;
}

// ---- building blocks (engine.hip) ------------------------------------------------------------------
double weight_bytes_per_element(const GptModel & m);
// layer l of the context's own KV cache of model m (one of c->gpt)
inline GptRun & run_of(bark_context * c, const GptModel & m) { return c->gpt_run[&m - c->gpt]; }
inline float * layer_k(bark_context * c, const GptModel & m, int l) { return run_of(c, m).kcache + m.kv_layer_stride * (size_t) l; }
inline float * layer_v(bark_context * c, const GptModel & m, int l) { return run_of(c, m).vcache + m.kv_layer_stride * (size_t) l; }
inline float * layer_vt(bark_context * c, const GptModel & m, int l) { float * vt = run_of(c, m).vtcache; return vt ? vt + m.kv_layer_stride * (size_t) l : nullptr; }
// the many-row scratch a forward pass works in: the context's own (P rows), or the fine batch's (several windows back to back)
struct RowBufs { float * x, * q; half_t * xn, * att, * hbuf, * q16, * k16, * vt16; float * logits; const int32_t * tokens; int plane; };
RowBufs own_rows(bark_context * c);
bool fine_products_on_f16_mfma(const bark_context * c, const GptModel & m, bool causal);
// marks a context as running a lock-step job / a side-by-side fine pass for the lifetime of the object (bark_context::fine_order's default policy)
struct JobScope {
    bark_context * c; bool prev;
    explicit JobScope(bark_context * ctx) : c(ctx), prev(ctx->in_job) { ctx->in_job = true; }
    ~JobScope() { c->in_job = prev; }
    JobScope(const JobScope &) = delete; JobScope & operator=(const JobScope &) = delete;
};
// seq > 0: the N rows are N / seq independent sequences (fine windows), sequence z with its cache at kbase / vbase + z * kv_seq_stride
// One of the four products of GPT layer l, with everything that follows from the model alone: W / wq, M, K, bias, epi (QKV also E and P, FC the GELU
// LUT) and in ln_g / ln_b the LayerNorm that belongs in front of it (ln1: QKV, ln2: FC).  The caller adds its input rows, outputs, N / slots, state and
// route; one that runs the LayerNorm as a launch of its own (rows already normalised) takes the pair from the descriptor and clears it.
enum LayerOp { OP_QKV = 0, OP_PROJ = 1, OP_FC = 2, OP_MPROJ = 3 };      // the `op` of the timing hooks
LinArgs layer_product(const bark_context * c, const GptModel & m, int l, int op);
// final LayerNorm + LM head on ONE row xrow (bark.cpp:1391-1405): rows [row0, row0 + n_rows) of the head, or the parity-selected codebook window
// of the coarse model (parity_rows, from st->step); logits -> out, rows ld_out apart
LinArgs lm_head_args(const GptModel & m, int row0, int n_rows, int parity_rows, const float * xrow, float * out, int ld_out, const StepState * st);
// the model half of EmbedArgs / SampleArgs: token and position tables of a causal model
template <typename Args> void set_token_embedding(Args & a, const bark_context * c, const GptModel & m) {
    a.wte = m.wte[0]; a.wte_q = m.wte_q[0]; a.wpe = m.wpe; a.E = m.hp.n_embd; a.n_in = m.hp.n_in_vocab; a.P = c->P;
}
void embed_state_row(bark_context * c, const GptModel & m, const StepState * st, float * x);      // x = embedding of st->cur_token at position st->n_past
// Stream capture -> executable graph: `body` enqueues its launches on s (capture mode: thread local).  A body that throws ends the capture - the
// stream would stay in capture mode for good otherwise - and what it recorded is dropped.  Runs once per graph, off the hot path.
GraphExec capture_graph(hipStream_t s, const std::function<void()> & body);
// device time of what `body` enqueues on the context's stream, in microseconds: a pair of events around it
double time_on_stream_us(bark_context * c, const std::function<void()> & body);
void run_layers_rows(bark_context * c, GptModel & m, int N, bool causal, float * kbase = nullptr, float * vbase = nullptr, int pos0 = 0,
                     const RowBufs * rb = nullptr, int seq = 0, size_t kv_seq_stride = 0, const SeqTab * seqtab = nullptr);
void run_layers_decode(bark_context * c, GptModel & m);
void run_lm_head(bark_context * c, GptModel & m, const float * xrow, int row0, int n_rows, int parity_rows, float out_div = 0.0f);
void set_state(bark_context * c, const StepState & st);
StepState get_state(bark_context * c);
StepState fresh_state();
void upload_tokens(bark_context * c, const int32_t * tok, size_t n);
void check_ids(const int32_t * tok, size_t n, int n_in, const char * what);
int run_prefill(bark_context * c, GptModel & m, int n_tokens, bool merge, float * kbase = nullptr, float * vbase = nullptr, int pos0 = 0);
struct StageCfg {            // what differs between the semantic and the coarse decode step
    int which; int mode; int lm_row0, lm_rows, parity_rows; int token_base; float min_eos_p; int eos_token; float temp;
};
StageCfg stage_cfg(bark_context * c, int which);
void run_sample(bark_context * c, const StageCfg & s, int n_past_add, bool prescaled = false);
void enqueue_decode_step(bark_context * c, const StageCfg & s, bool sample, int n_past_add, bool embed = true);
GraphExec capture_decode(bark_context * c, const StageCfg & s, int n_past_add, int n_steps = 1, int ng = 4);
void decode_steps_greedy(bark_context * c, const StageCfg & s, int n, int n_past);
int sample_host(std::vector<float> & l, std::mt19937 & rng, float temp, float * eos_p, const bark_hip_sampling_filter * flt = nullptr);
void filter_host(std::vector<float> & l, int32_t top_k, float top_p);      // C8n's cut, restated with a sort (removed ids -> -inf)
std::vector<float> fetch_logits(bark_context * c, size_t n);
void upload_uniforms(bark_context * c, int n);
void upload_filter(bark_context * c);
void consume_uniforms(bark_context * c, int n_used);
void progress(bark_context * c, bark_encoding_step step, int pct);
void run_fine_forward(bark_context * c, int nn, int n_rows, const RowBufs * rb = nullptr, int Z = 1);
// The fine stage's plan of one utterance (bark_eval_fine_encoder, bark.cpp:1961-2059): T frames in L = max(T, 1024) rows of in_arr [L][8], n_loops
// windows of 1024 rows with a hop of 512; window n reads rows from start_idx and keeps the picks of its positions >= rel (rows from start_fill_idx)
// With a voice prompt (C10v) its last n_hist <= 512 fine rows sit in front: L = max(n_hist + T, 1024), the fill starts at row n_hist, the result is rows
// n_hist .. n_hist + T (fine_plan_result)
struct FinePlan { int T = 0, L = 0, n_loops = 0, n_hist = 0; std::vector<int32_t> in_arr; };
struct FineWindow { int start_idx, start_fill_idx, rel; };
FinePlan fine_plan(const bark_context_params & p, const std::vector<int32_t> & coarse, const VoicePrompt * voice = nullptr);
std::vector<int32_t> fine_plan_result(FinePlan & f);
FineWindow fine_window(const FinePlan & f, int n);
// C10v.2: what the coarse stage keeps of a voice prompt - the last n_sh semantic ids and the last n_ch - 2 interleaved coarse ids as offset ids; both empty
// without a voice.  Throws when the trimmed history is empty (n_sh < 2 or n_ch <= 2).
struct VoiceTrim { std::vector<int32_t> sem, coarse; };
VoiceTrim voice_trim(const bark_context_params & p, const VoicePrompt * v);
// prompt of the coarse window that starts at step_idx (bark.cpp:1787-1807): 256 semantic ids from [history ; semantic] (padded), the infer token, the last
// max_coarse_history ids of [history ; out] (out: the offset ids generated so far)
std::vector<int32_t> coarse_window_prompt(const bark_context_params & p, const VoiceTrim & vt, const std::vector<int32_t> & semantic, const std::vector<int32_t> & out, int step_idx);
// window -> tok [8][plane] (this window's 1024 columns), and the picks of channels nc.. at positions >= rel back into in_arr
void fine_window_tokens(const FinePlan & f, const FineWindow & w, int32_t * tok, size_t plane);
void fine_write_back(FinePlan & f, const FineWindow & w, const bark_context_params & p, const int32_t * tok, size_t plane);
void ensure_fine_batch(bark_context * c, int Z);            // scratch of engine_fine_many for Z windows side by side
RowBufs fine_batch_rows(bark_context * c, int Z);

} }  // namespace barkhip::detail
