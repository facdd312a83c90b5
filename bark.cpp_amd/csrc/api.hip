// api.hip - C ABI of libbark.so: the reference's bark.h surface (drop-in) plus bark_mi355x.h.
// No exception crosses the boundary; failures are reported as nullptr / false / negative counts with
// a diagnostic on stderr, like the reference (bark.cpp:1174-1177, 2379-2401).
#include "engine.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <thread>
#include <vector>

using namespace barkhip;

#define HIP_OK_API(expr) do { if ((expr) != hipSuccess) throw std::runtime_error("HIP error at " #expr); } while (0)

namespace {
int64_t wall_us() {
    return std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
// noexcept shell of every entry point.  Kernel launches are not checked one by one (hipLaunchKernelGGL), so the sticky launch
// error is read here: a launch that was rejected means missing results, which must fail the call instead of returning them.
template <typename F> auto guarded(const char * what, decltype(std::declval<F>()()) fail, F && f, bool uses_gpu = true) -> decltype(f()) {
    try {
        if (!uses_gpu) return f();                                   // host-only entry points (bark_model_quantize) work without a device
        (void) hipGetLastError();
        auto r = f();
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) { fprintf(stderr, "%s: a kernel launch failed: %s\n", what, hipGetErrorString(e)); return fail; }
        return r;
    }
    catch (const std::exception & e) { fprintf(stderr, "%s: %s\n", what, e.what()); }
    catch (...) { fprintf(stderr, "%s: unknown failure\n", what); }
    return fail;
}
}  // namespace

extern "C" {

// defaults: /root/reference/bark.cpp:2202-2232
struct bark_context_params bark_context_default_params(void) {
    struct bark_context_params p;
    memset(&p, 0, sizeof(p));
    p.verbosity = LOW;
    p.temp = 0.7f;
    p.fine_temp = 0.5f;
    p.min_eos_p = 0.2f;
    p.sliding_window_size = 60;
    p.max_coarse_history = 630;
    p.sample_rate = 24000;
    p.target_bandwidth = 6;
    p.cls_token_id = 101;
    p.sep_token_id = 102;
    p.n_steps_text_encoder = 768;
    p.text_pad_token = 129595;
    p.text_encoding_offset = 10048;
    p.semantic_rate_hz = 49.9f;
    p.semantic_pad_token = 10000;
    p.semantic_vocab_size = 10000;
    p.semantic_infer_token = 129599;
    p.coarse_rate_hz = 75.0f;
    p.coarse_infer_token = 12050;
    p.coarse_semantic_pad_token = 12048;
    p.n_coarse_codebooks = 2;
    p.n_fine_codebooks = 8;
    p.codebook_size = 1024;
    p.progress_callback = nullptr;
    p.progress_callback_user_data = nullptr;
    return p;
}

struct bark_context * bark_load_model(const char * model_path, struct bark_context_params params, uint32_t seed) {
    const int64_t t0 = wall_us();
    if (!model_path) { fprintf(stderr, "bark_load_model: null path\n"); return nullptr; }
    bark_context * ctx = guarded("bark_load_model", (bark_context *) nullptr, [&] { return engine_load(model_path, params, seed); });
    if (ctx) ctx->stats.t_load_us = wall_us() - t0;
    return ctx;
}

bool bark_generate_audio(struct bark_context * bctx, const char * text, int n_threads) {
    (void) n_threads;      // CPU-backend hint in the reference (bark.cpp:1623-1625); the HIP engine has no use for it
    if (!bctx || !text) { fprintf(stderr, "bark_generate_audio: null argument\n"); return false; }
    return guarded("bark_generate_audio", false, [&] { return engine_generate(bctx, text); });
}

float * bark_get_audio_data(struct bark_context * bctx) { return (bctx && !bctx->audio.empty()) ? bctx->audio.data() : nullptr; }
int bark_get_audio_data_size(struct bark_context * bctx) { return bctx ? (int) bctx->audio.size() : 0; }
int64_t bark_get_load_time(struct bark_context * bctx) { return bctx ? bctx->stats.t_load_us : 0; }
int64_t bark_get_eval_time(struct bark_context * bctx) { return bctx ? bctx->stats.t_eval_us : 0; }

// Deviation from the reference, kept on purpose: bark.cpp:2403-2407 zeroes the WHOLE statistics struct and bark_generate_audio
// calls it first (bark.cpp:2131), so the reference's bark_get_load_time reads 0 after any generate call (examples/main prints "load time = 0.00 ms").
// Here the load time survives a reset: it describes the context, not a call.
void bark_reset_statistics(struct bark_context * bctx) {
    if (!bctx) return;
    const int64_t t_load = bctx->stats.t_load_us;
    bctx->stats = bark_hip_stats{};
    bctx->stats.t_load_us = t_load;
}

bool bark_model_quantize(const char * fname_inp, const char * fname_out, enum ggml_ftype ftype) {
    if (!fname_inp || !fname_out) { fprintf(stderr, "bark_model_quantize: null path\n"); return false; }
    return guarded("bark_model_quantize", false, [&] {
        std::string err;
        if (!model_quantize(fname_inp, fname_out, (int) ftype, err)) { fprintf(stderr, "bark_model_quantize: %s\n", err.c_str()); return false; }
        return true;
    }, /*uses_gpu=*/false);
}

void bark_free(struct bark_context * bctx) { delete bctx; }

// ---- ggml.h shim --------------------------------------------------------------------------------------
void ggml_time_init(void) {}
int64_t ggml_time_us(void) { return wall_us(); }
int64_t ggml_time_ms(void) { return wall_us() / 1000; }
struct ggml_context * ggml_init(struct ggml_init_params params) { (void) params; return nullptr; }
void ggml_free(struct ggml_context * ctx) { (void) ctx; }

// ---- bark_mi355x.h -------------------------------------------------------------------------------------
int bark_hip_hparams(struct bark_context * bctx, int which, int32_t * out10) {
    if (!bctx || which < 0 || which > 2 || !out10) return -1;
    const GptHparams & h = bctx->gpt[which].hp;
    const int32_t v[10] = {h.n_layer, h.n_head, h.n_embd, h.block_size, h.bias, h.n_in_vocab, h.n_out_vocab, h.n_lm_heads, h.n_wtes, h.ftype};
    memcpy(out10, v, sizeof(v));
    return 0;
}

void bark_hip_set_params(struct bark_context * bctx, struct bark_context_params params) {
    if (!bctx) return;
    bctx->params = params;
    guarded("bark_hip_set_params", 0, [&] { engine_invalidate_graphs(bctx); return 0; });   // sampling constants are baked into the graphs
}

int bark_hip_tokenize(struct bark_context * bctx, const char * text, int32_t * out513) {
    if (!bctx || !text || !out513) return -1;
    return guarded("bark_hip_tokenize", -1, [&] {
        PromptParams pp;
        pp.block_size = bctx->gpt[0].hp.block_size; pp.text_encoding_offset = bctx->params.text_encoding_offset;
        pp.text_pad_token = bctx->params.text_pad_token; pp.semantic_pad_token = bctx->params.semantic_pad_token;
        pp.semantic_infer_token = bctx->params.semantic_infer_token;
        std::vector<int32_t> ids = build_semantic_prompt(bctx->vocab, pp, text, false);
        engine_voice_into_prompt(bctx->params, bctx->voice.get(), ids);
        memcpy(out513, ids.data(), ids.size() * 4);
        return (int) ids.size();
    });
}

int bark_hip_bert_tokenize(struct bark_context * bctx, const char * text, int32_t * out, int n_max) {
    if (!bctx || !text || !out || n_max <= 0) return -1;
    return guarded("bark_hip_bert_tokenize", -1, [&] { return wordpiece_encode(bctx->vocab, text, out, n_max, false); });
}

int bark_hip_gpt_eval(struct bark_context * bctx, int which, const int32_t * tokens, int n_tokens, int n_past, int merge_ctx, float * logits) {
    if (!bctx || !tokens || !logits) return -1;
    return guarded("bark_hip_gpt_eval", -1, [&] { return engine_gpt_eval(bctx, which, tokens, n_tokens, n_past, merge_ctx != 0, logits); });
}

int bark_hip_fine_eval(struct bark_context * bctx, const int32_t * tokens_8x1024, int nn, float * logits) {
    if (!bctx || !tokens_8x1024 || !logits) return -1;
    return guarded("bark_hip_fine_eval", -1, [&] { engine_fine_eval(bctx, tokens_8x1024, nn, logits); return 0; });
}

int bark_hip_semantic(struct bark_context * bctx, const int32_t * prompt513, int32_t * out, int capacity, float * eos_trace) {
    if (!bctx || !prompt513 || !out || capacity < 0) return -1;
    return guarded("bark_hip_semantic", -1, [&] {
        std::vector<int32_t> prompt(prompt513, prompt513 + 513);
        std::vector<float> tr;
        std::vector<int32_t> r = engine_semantic(bctx, prompt, eos_trace ? &tr : nullptr);
        // the trace holds one entry per evaluated step: at most one more than the ids kept
        if ((int) r.size() > capacity || (eos_trace && (int) tr.size() > capacity + 1)) throw std::runtime_error("output buffer too small");
        if (!r.empty()) memcpy(out, r.data(), r.size() * 4);
        if (eos_trace && !tr.empty()) memcpy(eos_trace, tr.data(), tr.size() * 4);
        return (int) r.size();
    });
}

int bark_hip_coarse(struct bark_context * bctx, const int32_t * semantic, int n_semantic, int32_t * out_Tx2, int capacity_rows) {
    if (!bctx || !semantic || n_semantic <= 0 || !out_Tx2) return -1;
    return guarded("bark_hip_coarse", -1, [&] {
        std::vector<int32_t> r = engine_coarse(bctx, std::vector<int32_t>(semantic, semantic + n_semantic));
        if ((int) (r.size() / 2) > capacity_rows) throw std::runtime_error("output buffer too small");
        memcpy(out_Tx2, r.data(), r.size() * 4);
        return (int) r.size() / 2;
    });
}

int bark_hip_fine(struct bark_context * bctx, const int32_t * coarse_Tx2, int T, int32_t * out_Tx8, int capacity_rows) {
    if (!bctx || !coarse_Tx2 || T <= 0 || !out_Tx8) return -1;
    return guarded("bark_hip_fine", -1, [&] {
        std::vector<int32_t> r = engine_fine(bctx, std::vector<int32_t>(coarse_Tx2, coarse_Tx2 + (size_t) T * 2));
        if ((int) (r.size() / 8) > capacity_rows) throw std::runtime_error("output buffer too small");
        memcpy(out_Tx8, r.data(), r.size() * 4);
        return (int) r.size() / 8;
    });
}

int bark_hip_fine_many(struct bark_context * bctx, const int32_t * coarse_concat, const int * T, int n, int32_t * out_concat, int capacity_rows) {
    if (!bctx || !coarse_concat || !T || n <= 0 || n > 64 || !out_concat) return -1;          // 64 windows side by side: 270 MB of logits
    return guarded("bark_hip_fine_many", -1, [&] {
        std::vector<std::vector<int32_t>> co((size_t) n);
        std::vector<const std::vector<int32_t> *> ptr;
        std::vector<std::mt19937> rngs;
        size_t off = 0, total = 0;
        for (int i = 0; i < n; i++) {
            if (T[i] <= 0) throw std::runtime_error("fine_many: every utterance needs at least one frame");
            co[(size_t) i].assign(coarse_concat + off * 2, coarse_concat + (off + (size_t) T[i]) * 2);
            off += (size_t) T[i]; total += (size_t) T[i];
            ptr.push_back(&co[(size_t) i]);
            rngs.push_back(std::mt19937((uint32_t) bctx->rng()));
        }
        if ((long) total > (long) capacity_rows) throw std::runtime_error("output buffer too small");
        std::vector<std::vector<int32_t>> r = engine_fine_many(bctx, ptr, &rngs);
        off = 0;
        for (int i = 0; i < n; i++) { memcpy(out_concat + off * 8, r[(size_t) i].data(), r[(size_t) i].size() * 4); off += r[(size_t) i].size() / 8; }
        return (int) total;
    });
}

struct bark_context * bark_hip_load_model_on_device(const char * model_path, struct bark_context_params params, uint32_t seed, int device) {
    if (!model_path) { fprintf(stderr, "bark_hip_load_model_on_device: null path\n"); return nullptr; }
    if (device < 0) { fprintf(stderr, "bark_hip_load_model_on_device: negative device ordinal\n"); return nullptr; }
    const int64_t t0 = wall_us();
    bark_context * ctx = guarded("bark_hip_load_model_on_device", (bark_context *) nullptr, [&] { return engine_load(model_path, params, seed, device); });
    if (ctx) ctx->stats.t_load_us = wall_us() - t0;
    return ctx;
}

int bark_hip_set_fine_order(struct bark_context * bctx, int order) {
    if (!bctx || order < 0 || order > 2) return -1;
    return guarded("bark_hip_set_fine_order", -1, [&] {
        bctx->fine_order = order;
        if (bctx->tail) bctx->tail->fine_order = order;
        return 0;
    });
}

int bark_hip_codec_decode(struct bark_context * bctx, const int32_t * codes, int n_q, int T, float * pcm, int capacity) {
    if (!bctx || !codes || !pcm) return -1;
    return guarded("bark_hip_codec_decode", -1, [&] {
        std::vector<float> r = engine_codec_decode(bctx, codes, n_q, T, -1, nullptr);
        if ((int) r.size() > capacity) throw std::runtime_error("output buffer too small");
        memcpy(pcm, r.data(), r.size() * 4);
        return (int) r.size();
    });
}

int bark_hip_codec_decode_many(struct bark_context * bctx, const int32_t * const * codes, const int * T, int n, int n_q, float * pcm_concat, int capacity) {
    if (!bctx || !codes || !T || !pcm_concat || n <= 0 || n > 32) return -1;
    long total = 0;                                                 // refused before any work: a result that does not fit
    for (int i = 0; i < n; i++) { if (!codes[i]) return -1; total += T[i] > 0 ? 320L * T[i] : 0; }
    if (total > (long) capacity) return -1;
    return guarded("bark_hip_codec_decode_many", -1, [&] {
        std::vector<std::vector<float>> r = engine_codec_decode_many(bctx, std::vector<const int32_t *>(codes, codes + n), n_q, std::vector<int>(T, T + n), -1, nullptr);
        size_t off = 0;
        for (auto & v : r) {
            if (off + v.size() > (size_t) capacity) throw std::runtime_error("output buffer too small");
            memcpy(pcm_concat + off, v.data(), v.size() * 4); off += v.size();
        }
        return (int) off;
    });
}

int bark_hip_codec_tap(struct bark_context * bctx, const int32_t * codes, int n_q, int T, int stage, float * out, int capacity) {
    if (!bctx || !codes || !out) return -1;
    return guarded("bark_hip_codec_tap", -1, [&] {
        std::vector<float> tap;
        engine_codec_decode(bctx, codes, n_q, T, stage, &tap);
        if ((int) tap.size() > capacity) return -1;
        memcpy(out, tap.data(), tap.size() * 4);
        return (int) tap.size();
    });
}

int bark_hip_has_codec_encoder(struct bark_context * bctx) { return (bctx && bctx->codec.enc.present) ? 1 : 0; }

int bark_hip_codec_encode_many(struct bark_context * bctx, const float * const * pcm, const int * n_samples, int n, int n_q, int32_t * codes_concat, int capacity) {
    if (!bctx || !pcm || !n_samples || !codes_concat || n <= 0 || n > 32) return -1;
    for (int i = 0; i < n; i++) if (!pcm[i]) return -1;
    return guarded("bark_hip_codec_encode", -1, [&] {
        long total = 0;                                             // refused before any work: a result that does not fit
        for (int i = 0; i < n; i++) total += n_samples[i] > 0 ? (n_samples[i] + 319) / 320 : 0;
        if (n_q > 0 && total * n_q > (long) capacity) throw std::runtime_error("output buffer too small");
        std::vector<std::vector<int32_t>> r = engine_codec_encode_many(bctx, std::vector<const float *>(pcm, pcm + n), std::vector<int>(n_samples, n_samples + n), n_q, -1, nullptr);
        size_t off = 0;
        for (auto & v : r) { memcpy(codes_concat + off, v.data(), v.size() * 4); off += v.size(); }
        return (int) (off / (size_t) n_q);
    });
}

int bark_hip_codec_encode(struct bark_context * bctx, const float * pcm, int n_samples, int n_q, int32_t * codes, int capacity) {
    return bark_hip_codec_encode_many(bctx, &pcm, &n_samples, 1, n_q, codes, capacity);
}

int bark_hip_codec_encode_tap(struct bark_context * bctx, const float * pcm, int n_samples, int stage, float * out, int capacity) {
    if (!bctx || !pcm || !out || stage < 0) return -1;
    return guarded("bark_hip_codec_encode_tap", -1, [&] {
        std::vector<float> tap;
        engine_codec_encode_many(bctx, {pcm}, {n_samples}, 1, stage, &tap);
        if ((long) tap.size() > (long) capacity) return -1;
        memcpy(out, tap.data(), tap.size() * 4);
        return (int) tap.size();
    });
}

int bark_hip_codec_encode_latents(struct bark_context * bctx, float * out_TxH, int capacity) {
    if (!bctx || !out_TxH || !bctx->enc_latents) return -1;
    return guarded("bark_hip_codec_encode_latents", -1, [&] {
        const size_t n = (size_t) bctx->enc_latent_rows * (size_t) bctx->codec.hp.hidden_dim;
        if (n > (size_t) std::max(capacity, 0)) return -1;
        HIP_OK_API(hipSetDevice(bctx->device));
        HIP_OK_API(hipMemcpyAsync(out_TxH, bctx->enc_latents, n * 4, hipMemcpyDeviceToHost, bctx->stream));
        HIP_OK_API(hipStreamSynchronize(bctx->stream));
        return bctx->enc_latent_rows;
    });
}

double bark_hip_codec_encode_device_us(struct bark_context * bctx) { return bctx ? bctx->enc_device_us : -1.0; }

int bark_hip_rvq_encode(struct bark_context * bctx, const float * latents_TxH, int T, int n_q, int32_t * codes) {
    if (!bctx || !latents_TxH || !codes) return -1;
    return guarded("bark_hip_rvq_encode", -1, [&] {
        std::vector<int32_t> r = engine_rvq_encode(bctx, latents_TxH, T, n_q);
        memcpy(codes, r.data(), r.size() * 4);
        return T;
    });
}

int bark_hip_load_semantic_encoder(struct bark_context * bctx, const char * path) {
    if (!bctx || !path) return -1;
    return guarded("bark_hip_load_semantic_encoder", -1, [&] { engine_load_semantic_encoder(bctx, path); return 0; });
}

int bark_hip_has_semantic_encoder(struct bark_context * bctx) { return (bctx && bctx->hub) ? 1 : 0; }

int bark_hip_semantic_encode(struct bark_context * bctx, const float * pcm16k, int n_samples, int32_t * ids, int capacity) {
    if (!bctx || !pcm16k || !ids) return -1;
    return guarded("bark_hip_semantic_encode", -1, [&] {
        if (n_samples >= 400 && (n_samples - 400) / 320 + 1 > capacity) throw std::runtime_error("output buffer too small");      // refused before any work
        std::vector<int32_t> r = engine_semantic_encode(bctx, pcm16k, n_samples, -1, nullptr);
        memcpy(ids, r.data(), r.size() * 4);
        return (int) r.size();
    });
}

int bark_hip_semantic_encode_tap(struct bark_context * bctx, const float * pcm16k, int n_samples, int stage, float * out, int capacity) {
    if (!bctx || !pcm16k || !out || stage < 0) return -1;
    return guarded("bark_hip_semantic_encode_tap", -1, [&] {
        std::vector<float> tap;
        engine_semantic_encode(bctx, pcm16k, n_samples, stage, &tap);
        if ((long) tap.size() > (long) capacity) return -1;
        memcpy(out, tap.data(), tap.size() * 4);
        return (int) tap.size();
    });
}

int bark_hip_semantic_head(struct bark_context * bctx, const float * feats_TxH, int T, int32_t * ids, float * logits_or_null) {
    if (!bctx || !feats_TxH || !ids) return -1;
    return guarded("bark_hip_semantic_head", -1, [&] {
        std::vector<float> logits;
        std::vector<int32_t> r = engine_semantic_head(bctx, feats_TxH, T, logits_or_null ? &logits : nullptr);
        memcpy(ids, r.data(), r.size() * 4);
        if (logits_or_null) memcpy(logits_or_null, logits.data(), logits.size() * 4);
        return T;
    });
}

double bark_hip_semantic_encode_device_us(struct bark_context * bctx) { return bctx ? bctx->hub_device_us : -1.0; }

int bark_hip_resample_taps(float * out44) {
    if (!out44) return -1;
    memcpy(out44, resample_taps(), 44 * sizeof(float));
    return 44;
}

int bark_hip_resample_24k_to_16k(struct bark_context * bctx, const float * pcm24k, int n, float * out16k, int capacity) {
    if (!bctx || !pcm24k || !out16k) return -1;
    return guarded("bark_hip_resample_24k_to_16k", -1, [&] {
        if (n >= 1 && n <= kResampleMaxSamples && (2 * n + 2) / 3 > capacity) throw std::runtime_error("output buffer too small");      // refused before any work
        std::vector<float> r = engine_resample_24k_16k(bctx, pcm24k, n);
        memcpy(out16k, r.data(), r.size() * 4);
        return (int) r.size();
    });
}

double bark_hip_time_resample(struct bark_context * bctx, int n, int iters) {
    if (!bctx) return -1.0;
    return guarded("bark_hip_time_resample", -1.0, [&] { return engine_time_resample(bctx, n, iters); });
}

// ---- output rate and sample format (rule C14r) ----------------------------------------------------------------------------------------------------
int bark_hip_resample_out_len(int n, int rate_in, int rate_out) {
    const long long r = resample_out_len(n, rate_in, rate_out);
    return r < 0 || r > 0x7fffffffLL ? -1 : (int) r;
}

int bark_hip_resample_table(int rate_in, int rate_out, float * out, int capacity, int32_t lmh[3]) {
    return guarded("bark_hip_resample_table", -1, [&] {
        const ResampleTable * t = resample_pair_table(rate_in, rate_out);
        if (!t) return -1;
        if (lmh) { lmh[0] = t->L; lmh[1] = t->M; lmh[2] = t->half; }
        if (!out && capacity == 0) return (int) t->h.size();
        if (!out || (long) capacity < (long) t->h.size()) return -1;
        memcpy(out, t->h.data(), t->h.size() * sizeof(float));
        return (int) t->h.size();
    }, /*uses_gpu=*/false);
}

namespace {
// the bytes n segments give in `to`, or -1: a bad count / length / pair / format (what both resample calls refuse before any work)
long long resampled_bytes(const int * n, int count, int rate_in, const bark_hip_audio_format & to) {
    if (!n || count < 1 || count > kResampleMaxSegments || !sample_format_bytes(to.sample_format) || !resample_pair_supported(rate_in, to.sample_rate)) return -1;
    long long total = 0;
    for (int i = 0; i < count; i++) {
        if (n[i] < 1 || n[i] > kResampleMaxSamples) return -1;
        total += resample_out_len(n[i], rate_in, to.sample_rate) * sample_format_bytes(to.sample_format);
    }
    return total;
}
// BARK_HIP_SAMPLE_FLAC (rule C18f): a stream's length is known once it is made, so these routes render first and check the capacity against the real length
bool wants_flac(const struct bark_hip_audio_format * fmt) { return fmt && fmt->sample_format == BARK_HIP_SAMPLE_FLAC; }
int deliver(const std::vector<uint8_t> & r, void * out, int capacity_bytes) {
    if (r.size() > (size_t) 0x7ffffff0) return -1;
    if (!out || (size_t) std::max(capacity_bytes, 0) < r.size()) return -2 - (int) r.size();
    memcpy(out, r.data(), r.size());
    return (int) r.size();
}
// 24 kHz f32 samples held by the context -> `fmt`: the byte count, -(2 + bytes) if it does not fit, -1
int audio_as(struct bark_context * bctx, const char * what, const std::vector<float> & pcm, const struct bark_hip_audio_format * fmt, void * out, int capacity_bytes) {
    if (!fmt || pcm.empty()) return -1;
    const int n = (int) pcm.size();
    if (wants_flac(fmt)) {
        if (!resample_pair_supported(24000, fmt->sample_rate) || n > kResampleMaxSamples) return -1;
        return guarded(what, -1, [&] {
            const float * p = pcm.data();
            std::vector<int32_t> n_out;
            return deliver(engine_resample_many(bctx, &p, &n, 1, 24000, fmt->sample_rate, fmt->sample_format, n_out), out, capacity_bytes);
        });
    }
    const long long bytes = resampled_bytes(&n, 1, 24000, *fmt);
    if (bytes < 0 || bytes > 0x7ffffff0LL) return -1;
    if (!out || (long long) capacity_bytes < bytes) return -2 - (int) bytes;
    return guarded(what, -1, [&] {
        const float * p = pcm.data();
        std::vector<int32_t> n_out;
        const std::vector<uint8_t> r = engine_resample_many(bctx, &p, &n, 1, 24000, fmt->sample_rate, fmt->sample_format, n_out);
        memcpy(out, r.data(), r.size());
        return (int) r.size();
    });
}
}  // namespace

int bark_hip_resample_many(struct bark_context * bctx, const float * const * pcm, const int * n, int count, int rate_in, const struct bark_hip_audio_format * to,
                           void * out_concat, int capacity_bytes, int32_t * n_out) {
    if (!bctx || !pcm || !n || !to || !out_concat) return -1;
    const long long bytes = resampled_bytes(n, count, rate_in, *to);
    if (bytes < 0 || bytes > (long long) capacity_bytes) return -1;                       // refused before any work
    for (int i = 0; i < count; i++) if (!pcm[i]) return -1;
    return guarded("bark_hip_resample_many", -1, [&] {
        std::vector<int32_t> no;
        const std::vector<uint8_t> r = engine_resample_many(bctx, pcm, n, count, rate_in, to->sample_rate, to->sample_format, no);
        memcpy(out_concat, r.data(), r.size());
        if (n_out) memcpy(n_out, no.data(), no.size() * 4);
        return (int) r.size();
    });
}

int bark_hip_resample(struct bark_context * bctx, const float * pcm, int n, int rate_in, int rate_out, float * out, int capacity) {
    const bark_hip_audio_format to{rate_out, BARK_HIP_SAMPLE_F32};
    const long long cap_bytes = std::min<long long>(4LL * std::max(capacity, 0), 0x7ffffffcLL);
    const int r = bark_hip_resample_many(bctx, &pcm, &n, 1, rate_in, &to, out, (int) cap_bytes, nullptr);
    return r < 0 ? -1 : r / 4;
}

int bark_hip_get_audio_as(struct bark_context * bctx, const struct bark_hip_audio_format * fmt, void * out, int capacity_bytes) {
    if (!bctx) return -1;
    return audio_as(bctx, "bark_hip_get_audio_as", bctx->audio, fmt, out, capacity_bytes);
}

int bark_hip_batch_audio_as(struct bark_context * bctx, int i, const struct bark_hip_audio_format * fmt, void * out, int capacity_bytes) {
    if (!bctx || i < 0 || i >= (int) bctx->batch_results.size() || !bctx->batch_results[(size_t) i].ok) return -1;
    return audio_as(bctx, "bark_hip_batch_audio_as", bctx->batch_results[(size_t) i].audio, fmt, out, capacity_bytes);
}

double bark_hip_time_resample_pair(struct bark_context * bctx, int n, int rate_in, int rate_out, int sample_format, int iters) {
    if (!bctx) return -1.0;
    return guarded("bark_hip_time_resample_pair", -1.0, [&] { return engine_time_resample_pair(bctx, n, rate_in, rate_out, sample_format, iters); });
}

// ---- long-form text (rules C15s, C15j) ------------------------------------------------------------------------------------------------------------------
namespace {
bool join_call_valid(const int * n, int count, const bark_hip_join_params & p, const bark_hip_audio_format & to) {
    if (!n || count < 1 || count > kResampleMaxSegments || !join_params_valid(p) || !sample_format_bytes(to.sample_format) || !resample_pair_supported(24000, to.sample_rate)) return false;
    for (int i = 0; i < count; i++) if (n[i] < 1 || n[i] > kResampleMaxSamples) return false;
    return true;
}
// the joined audio of the context's long result in `to`, made once per format (the probe for the size and the call that fetches join once)
// speed != 1000 (rule C16t): the join runs over the time-scaled chunks - one tempo launch in front of it; lr.layout stays that of the chunks as generated
// loudness on (rule C17l): every chunk is levelled on its own, untrimmed, in front of the tempo - engine_level_many gives both; the cache key holds the request
void ensure_long_join(struct bark_context * bctx, const bark_hip_audio_format & to, int speed = 1000, const bark_hip_loudness_params & loud = bark_hip_loudness_params{0, 0.0f, 0.0f}) {
    bark_context::LongResult & lr = bctx->long_result;
    const bool same_loud = lr.joined_loudness.target_centilufs == loud.target_centilufs &&
                           (loud.target_centilufs == 0 || (lr.joined_loudness.peak_ceiling == loud.peak_ceiling && lr.joined_loudness.max_gain == loud.max_gain));
    if (lr.joined_fmt.sample_rate == to.sample_rate && lr.joined_fmt.sample_format == to.sample_format && lr.joined_speed == speed && same_loud) return;
    std::vector<const float *> pcm;
    std::vector<int> n;
    for (const bark_context::BatchResult & r : lr.chunks) { pcm.push_back(r.audio.data()); n.push_back((int) r.audio.size()); }
    lr.joined_fmt = bark_hip_audio_format{0, 0};
    lr.joined_info.clear();
    if (speed == 1000 && loud.target_centilufs == 0) lr.joined = engine_join_many(bctx, pcm.data(), n.data(), (int) n.size(), lr.join, to.sample_rate, to.sample_format, lr.layout);
    else {
        const std::vector<int32_t> sp(n.size(), speed);
        const std::vector<bark_hip_loudness_params> lp(n.size(), loud);
        std::vector<int32_t> n24, layout;
        const std::vector<uint8_t> scaled = loud.target_centilufs == 0
            ? engine_tempo_many(bctx, pcm.data(), n.data(), (int) n.size(), sp.data(), 24000, BARK_HIP_SAMPLE_F32, n24)
            : engine_level_many(bctx, pcm.data(), n.data(), (int) n.size(), lp.data(), sp.data(), 24000, BARK_HIP_SAMPLE_F32, n24, &lr.joined_info);
        size_t off = 0;
        for (size_t i = 0; i < n.size(); i++) { pcm[i] = reinterpret_cast<const float *>(scaled.data()) + off; n[i] = n24[i]; off += (size_t) n24[i]; }
        lr.joined = engine_join_many(bctx, pcm.data(), n.data(), (int) n.size(), lr.join, to.sample_rate, to.sample_format, layout);
    }
    lr.joined_fmt = to;
    lr.joined_speed = speed;
    lr.joined_loudness = loud;
}
}  // namespace

int bark_hip_split_text(struct bark_context * bctx, const char * text, int max_tokens, int32_t * spans_Nx2, int capacity_chunks) {
    if (!bctx || !text) return -1;
    return guarded("bark_hip_split_text", -1, [&] {
        const std::vector<TextSpan> spans = split_text(bctx->vocab, text, max_tokens);
        if ((int) spans.size() > capacity_chunks || (!spans.empty() && !spans_Nx2)) throw std::runtime_error("output buffer too small");
        for (size_t i = 0; i < spans.size(); i++) { spans_Nx2[2 * i] = spans[i].begin; spans_Nx2[2 * i + 1] = spans[i].end; }
        return (int) spans.size();
    }, /*uses_gpu=*/false);
}

int bark_hip_generate_long(struct bark_context * bctx, const char * text, const struct bark_hip_long_params * lp, const struct bark_hip_request_params * params,
                           const struct bark_hip_sampling_filter * filter, const struct bark_hip_voice_prompt * voice) {
    if (!bctx || !text) return -1;
    bctx->long_result = bark_context::LongResult();                   // whatever refuses or fails below, no earlier result stays behind
    if (filter && !filter_valid(*filter)) return -1;
    return guarded("bark_hip_generate_long", -1, [&] {
        const bark_hip_long_params def{0, 0, join_default_params()};
        const VoicePtr v = engine_make_voice(bctx, voice);
        return engine_generate_long(bctx, text, lp ? *lp : def, params, filter, voice ? &v : nullptr);
    });
}

int bark_hip_long_audio_as(struct bark_context * bctx, const struct bark_hip_audio_format * fmt, void * out, int capacity_bytes) {
    if (!bctx || bctx->long_result.chunks.empty()) return -1;
    const bark_hip_audio_format to = fmt ? *fmt : bark_hip_audio_format{24000, BARK_HIP_SAMPLE_F32};
    if (!render_format_bytes(to.sample_format) || !resample_pair_supported(24000, to.sample_rate)) return -1;
    return guarded("bark_hip_long_audio_as", -1, [&] {
        ensure_long_join(bctx, to);
        const std::vector<uint8_t> & r = bctx->long_result.joined;
        if (r.empty()) return 0;                                                          // every chunk trimmed away
        if (!out || (size_t) std::max(capacity_bytes, 0) < r.size()) return -2 - (int) r.size();
        memcpy(out, r.data(), r.size());
        return (int) r.size();
    });
}

int bark_hip_long_chunks(struct bark_context * bctx, int32_t * out_Nx4, int capacity_chunks) {
    if (!bctx || bctx->long_result.chunks.empty()) return -1;
    const int n = (int) bctx->long_result.chunks.size();
    if (!out_Nx4 || capacity_chunks < n) return -1;
    return guarded("bark_hip_long_chunks", -1, [&] {
        bark_context::LongResult & lr = bctx->long_result;
        if (lr.layout.empty()) {                                     // no join has run yet: the layout alone (one launch with a threshold, none without)
            std::vector<const float *> pcm;
            std::vector<int> len;
            for (const bark_context::BatchResult & r : lr.chunks) { pcm.push_back(r.audio.data()); len.push_back((int) r.audio.size()); }
            lr.layout = engine_join_layout(bctx, pcm.data(), len.data(), n, lr.join);
        }
        for (int i = 0; i < n; i++) {
            out_Nx4[4 * i] = lr.spans[(size_t) i].begin; out_Nx4[4 * i + 1] = lr.spans[(size_t) i].end;
            out_Nx4[4 * i + 2] = lr.layout[(size_t) i * 2]; out_Nx4[4 * i + 3] = lr.layout[(size_t) i * 2 + 1];
        }
        return n;
    });
}

int bark_hip_long_chunk_audio(struct bark_context * bctx, int i, float ** data) {
    if (!bctx || i < 0 || i >= (int) bctx->long_result.chunks.size()) return -1;
    if (data) *data = bctx->long_result.chunks[(size_t) i].audio.data();
    return (int) bctx->long_result.chunks[(size_t) i].audio.size();
}

int bark_hip_long_chunk_tokens(struct bark_context * bctx, int i, int stage, int32_t * out, int capacity) {
    if (!bctx || i < 0 || i >= (int) bctx->long_result.chunks.size() || stage < 0 || stage > 2) return -1;
    const auto & r = bctx->long_result.chunks[(size_t) i];
    const std::vector<int32_t> & v = stage == 0 ? r.semantic : stage == 1 ? r.coarse : r.fine;
    if (!out || capacity < (int) v.size()) return -1;
    if (!v.empty()) memcpy(out, v.data(), v.size() * 4);
    return (int) v.size();
}

int bark_hip_join_many(struct bark_context * bctx, const float * const * pcm, const int * n, int count, const struct bark_hip_join_params * params,
                       const struct bark_hip_audio_format * to, void * out, int capacity_bytes, int32_t * layout_Nx2) {
    if (!bctx || !pcm || !n) return -1;
    const bark_hip_join_params p = params ? *params : join_default_params();
    const bark_hip_audio_format f = to ? *to : bark_hip_audio_format{24000, BARK_HIP_SAMPLE_F32};
    if (!join_call_valid(n, count, p, f)) return -1;                                      // refused before any work
    for (int i = 0; i < count; i++) if (!pcm[i]) return -1;
    return guarded("bark_hip_join_many", -1, [&] {
        std::vector<int32_t> layout;
        const std::vector<uint8_t> r = engine_join_many(bctx, pcm, n, count, p, f.sample_rate, f.sample_format, layout);
        if (layout_Nx2) memcpy(layout_Nx2, layout.data(), layout.size() * 4);
        if (r.empty()) return 0;                                                          // every segment trimmed away
        if (!out || (size_t) std::max(capacity_bytes, 0) < r.size()) return -2 - (int) r.size();
        memcpy(out, r.data(), r.size());
        return (int) r.size();
    });
}

double bark_hip_time_join(struct bark_context * bctx, int count, int n_each, int rate_out, int sample_format, int iters) {
    if (!bctx) return -1.0;
    return guarded("bark_hip_time_join", -1.0, [&] { return engine_time_join(bctx, count, n_each, rate_out, sample_format, iters); });
}
double bark_hip_time_join_activity(struct bark_context * bctx, int count, int n_each, int iters) {
    if (!bctx) return -1.0;
    return guarded("bark_hip_time_join_activity", -1.0, [&] { return engine_time_join(bctx, count, n_each, 24000, BARK_HIP_SAMPLE_F32, iters, true); });
}

// ---- speaking rate (rule C16t) ----------------------------------------------------------------------------------------------------------------------------
namespace {
bool speed_valid(int p) { return p >= kTempoMinSpeed && p <= kTempoMaxSpeed; }
// the bytes the segments give at their speeds in `to`, or -1: what the tempo calls refuse before any work (the samples' values apart)
long long tempo_bytes(const int * n, const int32_t * speed, int count, const bark_hip_audio_format & to) {
    if (!n || !speed || count < 1 || count > kResampleMaxSegments || !sample_format_bytes(to.sample_format) || !resample_pair_supported(24000, to.sample_rate)) return -1;
    long long total = 0;
    for (int i = 0; i < count; i++) {
        const long long n24 = tempo_out_len(n[i], speed[i]);
        if (n24 < 0) return -1;
        total += resample_out_len(n24, 24000, to.sample_rate) * sample_format_bytes(to.sample_format);
    }
    return total;
}
// audio_as at a speaking rate: 24 kHz f32 samples held by the context -> C16t -> `fmt`
int audio_at(struct bark_context * bctx, const char * what, const std::vector<float> & pcm, const struct bark_hip_audio_format * fmt, int speed, void * out, int capacity_bytes) {
    if (!speed_valid(speed)) return -1;
    if (speed == 1000) return audio_as(bctx, what, pcm, fmt, out, capacity_bytes);
    if (!fmt || pcm.empty()) return -1;
    const int n = (int) pcm.size();
    const int32_t sp = speed;
    if (wants_flac(fmt)) {
        if (!resample_pair_supported(24000, fmt->sample_rate) || tempo_out_len(n, speed) < 0) return -1;
        return guarded(what, -1, [&] {
            const float * p = pcm.data();
            std::vector<int32_t> n_out;
            return deliver(engine_tempo_many(bctx, &p, &n, 1, &sp, fmt->sample_rate, fmt->sample_format, n_out), out, capacity_bytes);
        });
    }
    const long long bytes = tempo_bytes(&n, &sp, 1, *fmt);
    if (bytes < 0 || bytes > 0x7ffffff0LL) return -1;
    if (!out || (long long) capacity_bytes < bytes) return -2 - (int) bytes;
    return guarded(what, -1, [&] {
        const float * p = pcm.data();
        std::vector<int32_t> n_out;
        const std::vector<uint8_t> r = engine_tempo_many(bctx, &p, &n, 1, &sp, fmt->sample_rate, fmt->sample_format, n_out);
        memcpy(out, r.data(), r.size());
        return (int) r.size();
    });
}
}  // namespace

int bark_hip_tempo_out_len(int n, int speed_permille) { return (int) tempo_out_len(n, speed_permille); }

int bark_hip_tempo_window(float * out720) {
    if (!out720) return -1;
    memcpy(out720, tempo_window(), kTempoFrame * sizeof(float));
    return kTempoFrame;
}

int bark_hip_tempo_many(struct bark_context * bctx, const float * const * pcm, const int * n, int count, const int32_t * speed_permille, const struct bark_hip_audio_format * to,
                        void * out_concat, int capacity_bytes, int32_t * n_out) {
    if (!bctx || !pcm || !n || !speed_permille || !out_concat) return -1;
    const bark_hip_audio_format f = to ? *to : bark_hip_audio_format{24000, BARK_HIP_SAMPLE_F32};
    const long long bytes = tempo_bytes(n, speed_permille, count, f);
    if (bytes < 0 || bytes > (long long) capacity_bytes) return -1;                       // refused before any work
    for (int i = 0; i < count; i++) if (!pcm[i]) return -1;
    return guarded("bark_hip_tempo_many", -1, [&] {
        std::vector<int32_t> no;
        const std::vector<uint8_t> r = engine_tempo_many(bctx, pcm, n, count, speed_permille, f.sample_rate, f.sample_format, no);
        memcpy(out_concat, r.data(), r.size());
        if (n_out) memcpy(n_out, no.data(), no.size() * 4);
        return (int) r.size();
    });
}

int bark_hip_tempo(struct bark_context * bctx, const float * pcm, int n, int speed_permille, float * out, int capacity) {
    const int32_t sp = speed_permille;
    const long long cap_bytes = std::min<long long>(4LL * std::max(capacity, 0), 0x7ffffffcLL);
    const int r = bark_hip_tempo_many(bctx, &pcm, &n, 1, &sp, nullptr, out, (int) cap_bytes, nullptr);
    return r < 0 ? -1 : r / 4;
}

int bark_hip_tempo_positions(struct bark_context * bctx, const float * pcm, int n, int speed_permille, int32_t * pos, int capacity) {
    if (!bctx || !pcm || !pos) return -1;
    const long long n24 = tempo_out_len(n, speed_permille);
    if (n24 < 0 || (n24 + kTempoHop - 1) / kTempoHop > (long long) capacity) return -1;
    return guarded("bark_hip_tempo_positions", -1, [&] {
        const int32_t sp = speed_permille;
        std::vector<int32_t> no, positions;
        engine_tempo_many(bctx, &pcm, &n, 1, &sp, 24000, BARK_HIP_SAMPLE_F32, no, &positions);
        memcpy(pos, positions.data(), positions.size() * 4);
        return (int) positions.size();
    });
}

int bark_hip_get_audio_at(struct bark_context * bctx, const struct bark_hip_audio_format * fmt, int speed_permille, void * out, int capacity_bytes) {
    if (!bctx) return -1;
    return audio_at(bctx, "bark_hip_get_audio_at", bctx->audio, fmt, speed_permille, out, capacity_bytes);
}

int bark_hip_batch_audio_at(struct bark_context * bctx, int i, const struct bark_hip_audio_format * fmt, int speed_permille, void * out, int capacity_bytes) {
    if (!bctx || i < 0 || i >= (int) bctx->batch_results.size() || !bctx->batch_results[(size_t) i].ok) return -1;
    return audio_at(bctx, "bark_hip_batch_audio_at", bctx->batch_results[(size_t) i].audio, fmt, speed_permille, out, capacity_bytes);
}

int bark_hip_long_audio_at(struct bark_context * bctx, const struct bark_hip_audio_format * fmt, int speed_permille, void * out, int capacity_bytes) {
    if (!speed_valid(speed_permille)) return -1;
    if (speed_permille == 1000) return bark_hip_long_audio_as(bctx, fmt, out, capacity_bytes);
    if (!bctx || bctx->long_result.chunks.empty()) return -1;
    const bark_hip_audio_format to = fmt ? *fmt : bark_hip_audio_format{24000, BARK_HIP_SAMPLE_F32};
    if (!render_format_bytes(to.sample_format) || !resample_pair_supported(24000, to.sample_rate)) return -1;
    return guarded("bark_hip_long_audio_at", -1, [&] {
        ensure_long_join(bctx, to, speed_permille);
        const std::vector<uint8_t> & r = bctx->long_result.joined;
        if (r.empty()) return 0;                                                          // every chunk trimmed away
        if (!out || (size_t) std::max(capacity_bytes, 0) < r.size()) return -2 - (int) r.size();
        memcpy(out, r.data(), r.size());
        return (int) r.size();
    });
}

double bark_hip_time_tempo(struct bark_context * bctx, int count, int n_each, int speed_permille, int iters) {
    if (!bctx) return -1.0;
    return guarded("bark_hip_time_tempo", -1.0, [&] { return engine_time_tempo(bctx, count, n_each, speed_permille, iters); });
}

// ---- loudness (rule C17l) ---------------------------------------------------------------------------------------------------------------------------------
namespace {
const bark_hip_loudness_info kLoudnessOffInfo{0.0, 0.0, 0.0f, 1.0f, 0, 0, 0, 0};
bool render_valid(const bark_hip_audio_render & h) { return speed_valid(h.speed_permille) && loudness_params_valid(h.loudness); }
// audio_at with levelling: 24 kHz f32 samples held by the context -> C17l -> C16t -> `fmt`
int audio_with(struct bark_context * bctx, const char * what, const std::vector<float> & pcm, const struct bark_hip_audio_render * how, void * out, int capacity_bytes,
               struct bark_hip_loudness_info * info) {
    if (!how || !render_valid(*how)) return -1;
    if (how->loudness.target_centilufs == 0) {
        const int r = audio_at(bctx, what, pcm, &how->fmt, how->speed_permille, out, capacity_bytes);
        if (info && r != -1) *info = kLoudnessOffInfo;
        return r;
    }
    if (pcm.empty()) return -1;
    const int n = (int) pcm.size();
    const int32_t sp = how->speed_permille;
    if (wants_flac(&how->fmt)) {
        if (!resample_pair_supported(24000, how->fmt.sample_rate) || tempo_out_len(n, sp) < 0) return -1;
        return guarded(what, -1, [&] {
            const float * p = pcm.data();
            std::vector<int32_t> n_out;
            std::vector<bark_hip_loudness_info> inf;
            const std::vector<uint8_t> r = engine_level_many(bctx, &p, &n, 1, &how->loudness, &sp, how->fmt.sample_rate, how->fmt.sample_format, n_out, &inf);
            if (info) *info = inf[0];
            return deliver(r, out, capacity_bytes);
        });
    }
    const long long bytes = tempo_bytes(&n, &sp, 1, how->fmt);
    if (bytes < 0 || bytes > 0x7ffffff0LL) return -1;
    if (!out || (long long) capacity_bytes < bytes) return -2 - (int) bytes;
    return guarded(what, -1, [&] {
        const float * p = pcm.data();
        std::vector<int32_t> n_out;
        std::vector<bark_hip_loudness_info> inf;
        const std::vector<uint8_t> r = engine_level_many(bctx, &p, &n, 1, &how->loudness, &sp, how->fmt.sample_rate, how->fmt.sample_format, n_out, &inf);
        memcpy(out, r.data(), r.size());
        if (info) *info = inf[0];
        return (int) r.size();
    });
}
}  // namespace

int bark_hip_loudness_constants(double * out9) {
    if (!out9) return -1;
    memcpy(out9, loudness_constants(), 9 * sizeof(double));
    return 9;
}

double bark_hip_loudness_target_ms(int target_centilufs) {
    return target_centilufs >= kLoudMinTarget && target_centilufs <= kLoudMaxTarget ? loudness_target_ms(target_centilufs) : -1.0;
}

namespace {
// what the loudness calls refuse before any work (the samples' values apart)
bool loudness_call_valid(const float * const * pcm, const int * n, int count, const bark_hip_loudness_params * params) {
    if (!pcm || !n || count < 1 || count > kResampleMaxSegments) return false;
    for (int i = 0; i < count; i++) if (!pcm[i] || n[i] < 1 || n[i] > kResampleMaxSamples || (params && !loudness_params_valid(params[i]))) return false;
    return true;
}
}  // namespace

int bark_hip_loudness_many(struct bark_context * bctx, const float * const * pcm, const int * n, int count, const struct bark_hip_loudness_params * params,
                           struct bark_hip_loudness_info * info) {
    if (!bctx || !info || !loudness_call_valid(pcm, n, count, params)) return -1;
    return guarded("bark_hip_loudness_many", -1, [&] {
        const std::vector<bark_hip_loudness_info> r = engine_loudness_many(bctx, pcm, n, count, params);
        memcpy(info, r.data(), r.size() * sizeof(bark_hip_loudness_info));
        return count;
    });
}

int bark_hip_loudness_hops(struct bark_context * bctx, const float * pcm, int n, double * z, int capacity) {
    if (!bctx || !loudness_call_valid(&pcm, &n, 1, nullptr) || n / kLoudHop > capacity || (n >= kLoudHop && !z)) return -1;
    return guarded("bark_hip_loudness_hops", -1, [&] {
        std::vector<double> zs;
        engine_loudness_many(bctx, &pcm, &n, 1, nullptr, &zs);
        if (!zs.empty()) memcpy(z, zs.data(), zs.size() * sizeof(double));
        return (int) zs.size();
    });
}

int bark_hip_level_many(struct bark_context * bctx, const float * const * pcm, const int * n, int count, const struct bark_hip_loudness_params * params,
                        const int32_t * speed_permille, const struct bark_hip_audio_format * to, void * out_concat, int capacity_bytes, int32_t * n_out,
                        struct bark_hip_loudness_info * info) {
    if (!bctx || !params || !out_concat || !loudness_call_valid(pcm, n, count, params)) return -1;
    const bark_hip_audio_format f = to ? *to : bark_hip_audio_format{24000, BARK_HIP_SAMPLE_F32};
    const std::vector<int32_t> unit((size_t) count, 1000);
    const int32_t * sp = speed_permille ? speed_permille : unit.data();
    const long long bytes = tempo_bytes(n, sp, count, f);
    if (bytes < 0 || bytes > (long long) capacity_bytes) return -1;                       // refused before any work
    return guarded("bark_hip_level_many", -1, [&] {
        std::vector<int32_t> no;
        std::vector<bark_hip_loudness_info> inf;
        const std::vector<uint8_t> r = engine_level_many(bctx, pcm, n, count, params, sp, f.sample_rate, f.sample_format, no, &inf);
        memcpy(out_concat, r.data(), r.size());
        if (n_out) memcpy(n_out, no.data(), no.size() * 4);
        if (info) memcpy(info, inf.data(), inf.size() * sizeof(bark_hip_loudness_info));
        return (int) r.size();
    });
}

int bark_hip_get_audio_with(struct bark_context * bctx, const struct bark_hip_audio_render * how, void * out, int capacity_bytes, struct bark_hip_loudness_info * info) {
    if (!bctx) return -1;
    return audio_with(bctx, "bark_hip_get_audio_with", bctx->audio, how, out, capacity_bytes, info);
}

int bark_hip_batch_audio_with(struct bark_context * bctx, int i, const struct bark_hip_audio_render * how, void * out, int capacity_bytes, struct bark_hip_loudness_info * info) {
    if (!bctx || i < 0 || i >= (int) bctx->batch_results.size() || !bctx->batch_results[(size_t) i].ok) return -1;
    return audio_with(bctx, "bark_hip_batch_audio_with", bctx->batch_results[(size_t) i].audio, how, out, capacity_bytes, info);
}

int bark_hip_long_audio_with(struct bark_context * bctx, const struct bark_hip_audio_render * how, void * out, int capacity_bytes, struct bark_hip_loudness_info * info,
                             int info_capacity) {
    if (!how || !render_valid(*how)) return -1;
    if (!bctx || bctx->long_result.chunks.empty()) return -1;
    const size_t n_chunks = bctx->long_result.chunks.size();
    if (info && (size_t) std::max(info_capacity, 0) < n_chunks) return -1;
    if (how->loudness.target_centilufs == 0) {
        const int r = bark_hip_long_audio_at(bctx, &how->fmt, how->speed_permille, out, capacity_bytes);
        if (info && r != -1) for (size_t i = 0; i < n_chunks; i++) info[i] = kLoudnessOffInfo;
        return r;
    }
    const bark_hip_audio_format to = how->fmt;
    if (!render_format_bytes(to.sample_format) || !resample_pair_supported(24000, to.sample_rate)) return -1;
    return guarded("bark_hip_long_audio_with", -1, [&] {
        ensure_long_join(bctx, to, how->speed_permille, how->loudness);
        const bark_context::LongResult & lr = bctx->long_result;
        if (info) memcpy(info, lr.joined_info.data(), lr.joined_info.size() * sizeof(bark_hip_loudness_info));
        const std::vector<uint8_t> & r = lr.joined;
        if (r.empty()) return 0;                                                          // every chunk trimmed away
        if (!out || (size_t) std::max(capacity_bytes, 0) < r.size()) return -2 - (int) r.size();
        memcpy(out, r.data(), r.size());
        return (int) r.size();
    });
}

// ---- FLAC (rule C18f) ---------------------------------------------------------------------------------------------------------------------------------------
int bark_hip_flac_max_bytes(int n) {
    const long long b = flac_max_bytes(n);
    return b < 0 || b > 0x7ffffff0LL ? -1 : (int) b;
}

namespace {
// what the FLAC calls refuse before any work
bool flac_call_valid(const int16_t * const * pcm, const int * n, int count, int rate) {
    if (!pcm || !n || count < 1 || count > kResampleMaxSegments || !flac_rate_code(rate)) return false;
    long long bound = 0;
    for (int i = 0; i < count; i++) {
        if (!pcm[i] || flac_max_bytes(n[i]) < 0) return false;
        bound += flac_max_bytes(n[i]);
    }
    return bound <= 0x7ffffff0LL;
}
}  // namespace

int bark_hip_flac_encode_many(struct bark_context * bctx, const int16_t * const * pcm, const int * n, int count, int rate, void * out, int capacity_bytes, int32_t * lengths) {
    if (!bctx || !flac_call_valid(pcm, n, count, rate)) return -1;
    return guarded("bark_hip_flac_encode_many", -1, [&] {
        std::vector<int32_t> len;
        const std::vector<uint8_t> r = engine_flac_encode_many(bctx, pcm, n, count, rate, len);
        if (lengths) memcpy(lengths, len.data(), len.size() * 4);
        return deliver(r, out, capacity_bytes);
    });
}

int bark_hip_flac_frames(struct bark_context * bctx, const int16_t * pcm, int n, int rate, int32_t * out_Nx4, int capacity_frames) {
    if (!bctx || !out_Nx4 || !flac_call_valid(&pcm, &n, 1, rate) || (long long) capacity_frames < ((long long) n + kFlacBlock - 1) / kFlacBlock) return -1;
    return guarded("bark_hip_flac_frames", -1, [&] {
        std::vector<int32_t> len, frames;
        engine_flac_encode_many(bctx, &pcm, &n, 1, rate, len, &frames);
        memcpy(out_Nx4, frames.data(), frames.size() * 4);
        return (int) (frames.size() / 4);
    });
}

double bark_hip_time_flac(struct bark_context * bctx, int count, int n_each, int iters) {
    if (!bctx) return -1.0;
    return guarded("bark_hip_time_flac", -1.0, [&] { return engine_time_flac(bctx, count, n_each, iters); });
}
double bark_hip_time_flac_launch(struct bark_context * bctx, int count, int n_each, int which, int iters) {
    if (!bctx || which < 1 || which > 2) return -1.0;
    return guarded("bark_hip_time_flac_launch", -1.0, [&] { return engine_time_flac(bctx, count, n_each, iters, which); });
}

double bark_hip_time_loudness(struct bark_context * bctx, int count, int n_each, int level, int iters) {
    if (!bctx) return -1.0;
    return guarded("bark_hip_time_loudness", -1.0, [&] { return engine_time_loudness(bctx, count, n_each, iters, level != 0); });
}

namespace {
// the part of a recording that bark_hip_voice_from_audio uses, and the sizes of what it makes of it
struct VoiceAudioCounts { int n_used, n_sem, n_frames; };
VoiceAudioCounts voice_audio_counts(int n_samples) {
    VoiceAudioCounts k;
    k.n_used = std::min(n_samples, BARK_HIP_VOICE_AUDIO_MAX_SAMPLES);
    k.n_sem = ((2 * k.n_used + 2) / 3 - 400) / 320 + 1;
    k.n_frames = (k.n_used + 319) / 320;
    return k;
}
}  // namespace

int bark_hip_voice_from_audio(struct bark_context * bctx, const float * pcm24k, int n_samples, int32_t * semantic, int semantic_capacity, int32_t * coarse_Tx2,
                              int32_t * fine_Tx8, int capacity_rows, int32_t * n_semantic, int32_t * n_frames) {
    if (!bctx || !pcm24k || !semantic || !coarse_Tx2 || !fine_Tx8 || !n_semantic || !n_frames) return -1;
    return guarded("bark_hip_voice_from_audio", -1, [&] {
        if (n_samples >= 599) {                                     // refused before any work: a result that does not fit
            const VoiceAudioCounts k = voice_audio_counts(n_samples);
            if (k.n_sem > semantic_capacity || k.n_frames > capacity_rows) throw std::runtime_error("output buffer too small");
        }
        const VoicePtr v = engine_voice_from_audio(bctx, pcm24k, n_samples);
        memcpy(semantic, v->semantic.data(), v->semantic.size() * 4);
        memcpy(coarse_Tx2, v->coarse.data(), v->coarse.size() * 4);
        memcpy(fine_Tx8, v->fine.data(), v->fine.size() * 4);
        *n_semantic = (int32_t) v->semantic.size();
        *n_frames = (int32_t) (v->fine.size() / 8);
        return 0;
    });
}

int bark_hip_set_voice_from_audio(struct bark_context * bctx, const float * pcm24k, int n_samples) {
    if (!bctx || !pcm24k) return -1;
    return guarded("bark_hip_set_voice_from_audio", -1, [&] {
        VoicePtr v = engine_voice_from_audio(bctx, pcm24k, n_samples);      // throws on a refusal: the context keeps what it had
        bctx->voice = v;
        return 0;
    });
}

struct bark_context * bark_hip_clone_context(struct bark_context * src, uint32_t seed) {
    if (!src) return nullptr;
    return guarded("bark_hip_clone_context", (bark_context *) nullptr, [&] { return engine_clone(src, seed); });
}

int bark_hip_generate_audio_batch(struct bark_context ** ctxs, const char * const * texts, int n) {
    if (!ctxs || !texts || n <= 0) return 0;
    std::vector<char> ok((size_t) n, 0);
    std::vector<std::thread> th;
    for (int i = 0; i < n; i++)
        th.emplace_back([&, i] { ok[(size_t) i] = (ctxs[i] && texts[i]) ? (char) guarded("bark_hip_generate_audio_batch", false, [&] { return engine_generate(ctxs[i], texts[i]); }) : 0; });
    for (auto & t : th) t.join();
    int good = 0;
    for (char c : ok) good += c;
    return good;
}

int bark_hip_generate_batch(struct bark_context * bctx, const char * const * texts, int n) {
    if (!bctx || !texts || n <= 0) return -1;
    for (int i = 0; i < n; i++) if (!texts[i]) return -1;
    return guarded("bark_hip_generate_batch", -1, [&] { return engine_generate_batch(bctx, texts, n, nullptr); });
}
int bark_hip_generate_batch_seeded(struct bark_context * bctx, const char * const * texts, int n, const uint32_t * seeds) {
    if (!bctx || !texts || !seeds || n <= 0) return -1;
    for (int i = 0; i < n; i++) if (!texts[i]) return -1;
    return guarded("bark_hip_generate_batch_seeded", -1, [&] { return engine_generate_batch(bctx, texts, n, seeds); });
}
int bark_hip_generate_batch_ex(struct bark_context * bctx, const char * const * texts, int n, const struct bark_hip_request_params * per_utterance) {
    if (!bctx || !texts || !per_utterance || n <= 0) return -1;
    for (int i = 0; i < n; i++) if (!texts[i]) return -1;
    return guarded("bark_hip_generate_batch_ex", -1, [&] { return engine_generate_batch(bctx, texts, n, nullptr, per_utterance); });
}
int bark_hip_generate_batch_filtered(struct bark_context * bctx, const char * const * texts, int n, const struct bark_hip_request_params * per_utterance,
                                     const struct bark_hip_sampling_filter * filters) {
    if (!bctx || !texts || n <= 0) return -1;
    for (int i = 0; i < n; i++) if (!texts[i]) return -1;
    if (filters) for (int i = 0; i < n; i++) if (!filter_valid(filters[i])) return -1;
    return guarded("bark_hip_generate_batch_filtered", -1, [&] { return engine_generate_batch(bctx, texts, n, nullptr, per_utterance, nullptr, filters); });
}
int bark_hip_set_sampling_filter(struct bark_context * bctx, int32_t top_k, float top_p) {
    const bark_hip_sampling_filter f{top_k, top_p};
    if (!bctx || !filter_valid(f)) return -1;
    return guarded("bark_hip_set_sampling_filter", -1, [&] {
        if (filter_on(f) != filter_on(bctx->filter)) engine_invalidate_graphs(bctx);       // the decode graphs hold the filter launch or not
        bctx->filter = f;
        return 0;
    });
}
int bark_hip_set_voice_prompt(struct bark_context * bctx, const struct bark_hip_voice_prompt * voice) {
    if (!bctx) return -1;
    return guarded("bark_hip_set_voice_prompt", -1, [&] {
        VoicePtr v = engine_make_voice(bctx, voice);          // throws on a bad one: the context keeps what it had
        bctx->voice = v;
        return 0;
    }, /*uses_gpu=*/false);
}
int bark_hip_generate_batch_voiced(struct bark_context * bctx, const char * const * texts, int n, const struct bark_hip_request_params * per_utterance,
                                   const struct bark_hip_sampling_filter * filters, const struct bark_hip_voice_prompt * const * voices) {
    if (!bctx || !texts || n <= 0) return -1;
    for (int i = 0; i < n; i++) if (!texts[i]) return -1;
    if (filters) for (int i = 0; i < n; i++) if (!filter_valid(filters[i])) return -1;
    return guarded("bark_hip_generate_batch_voiced", -1, [&] {
        std::vector<VoicePtr> vs;
        if (voices) for (int i = 0; i < n; i++) vs.push_back(engine_make_voice(bctx, voices[i]));
        return engine_generate_batch(bctx, texts, n, nullptr, per_utterance, nullptr, filters, voices ? vs.data() : nullptr);
    });
}
int bark_hip_pick_rows(struct bark_context * bctx, const float * logits, int n_windows, int n_cols, float temp, const double * u, const int32_t * rel,
                       int32_t * tokens_io, int32_t * near_ties) {
    if (!bctx || !logits || !rel || !tokens_io) return -1;
    return guarded("bark_hip_pick_rows", -1, [&] { engine_pick_rows(bctx, logits, n_windows, n_cols, temp, u, rel, tokens_io, near_ties); return 0; });
}
int bark_hip_sample_rows_filtered(struct bark_context * bctx, const float * logits, int n_rows, int n, const float * temp, const int32_t * top_k,
                                  const float * top_p, const double * u, int32_t * out_ids, float * out_eos_p) {
    if (!bctx || !logits || !temp || !top_k || !top_p || !u || !out_ids || n_rows <= 0) return -1;
    return guarded("bark_hip_sample_rows_filtered", -1, [&] { engine_sample_rows_filtered(bctx, logits, n_rows, n, temp, top_k, top_p, u, out_ids, out_eos_p); return 0; });
}
int bark_hip_sample_rows_state(struct bark_context * bctx, const float * logits, int n_rows, int n, const float * temp, const int32_t * top_k,
                               const float * top_p, const double * u, const float * min_eos_p, const struct bark_hip_sample_call * call,
                               int32_t * state_io, int32_t * out_ids, float * out_eos_p) {
    if (!bctx || !logits || !temp || !top_k || !top_p || !u || !min_eos_p || !call || !state_io || !out_ids || n_rows <= 0) return -1;
    return guarded("bark_hip_sample_rows_state", -1, [&] {
        engine_sample_rows_state(bctx, logits, n_rows, n, temp, top_k, top_p, u, min_eos_p, *call, state_io, out_ids, out_eos_p); return 0; });
}
double bark_hip_time_sample_filter(struct bark_context * bctx, int n, int n_slots, int32_t top_k, float top_p, int peaked, int iters) {
    if (!bctx) return -1.0;
    return guarded("bark_hip_time_sample_filter", -1.0, [&] { return engine_time_sample_filtered(bctx, n, n_slots, top_k, top_p, peaked, iters); });
}
int bark_hip_profile_lock_step(struct bark_context * bctx, int which, int n_slots, int ctx, int reps, char * json_out, int capacity) {
    if (!bctx || !json_out || capacity < 2) return -1;
    return guarded("bark_hip_profile_lock_step", -1, [&] {
        std::vector<std::pair<std::string, double>> tl;
        engine_profile_lock_step(bctx, which, n_slots, ctx, reps, tl);
        std::string js = "[";
        for (size_t i = 0; i < tl.size(); i++) {
            char buf[160];
            snprintf(buf, sizeof(buf), "%s{\"site\": \"%s\", \"us\": %.3f}", i ? ", " : "", tl[i].first.c_str(), tl[i].second);
            js += buf;
        }
        js += "]";
        if ((int) js.size() + 1 > capacity) return -1;
        memcpy(json_out, js.c_str(), js.size() + 1);
        return (int) js.size();
    });
}
int bark_hip_reserve_batch(struct bark_context * bctx, int slots) {
    if (!bctx) return -1;
    return guarded("bark_hip_reserve_batch", -1, [&] { engine_reserve_batch(bctx, slots); return 0; });
}
int bark_hip_batch_audio(struct bark_context * bctx, int i, float ** data) {
    if (!bctx || i < 0 || i >= (int) bctx->batch_results.size() || !bctx->batch_results[(size_t) i].ok) return -1;
    if (data) *data = bctx->batch_results[(size_t) i].audio.data();
    return (int) bctx->batch_results[(size_t) i].audio.size();
}
int bark_hip_batch_tokens(struct bark_context * bctx, int i, int stage, int32_t * out, int capacity) {
    if (!bctx || i < 0 || i >= (int) bctx->batch_results.size() || stage < 0 || stage > 2) return -1;
    const auto & r = bctx->batch_results[(size_t) i];
    const std::vector<int32_t> & v = stage == 0 ? r.semantic : stage == 1 ? r.coarse : r.fine;
    if (!out || capacity < (int) v.size()) return -1;
    if (!v.empty()) memcpy(out, v.data(), v.size() * 4);
    return (int) v.size();
}
int bark_hip_batch_lock_steps(struct bark_context * bctx, int32_t out2[2]) {
    if (!bctx || !out2 || bctx->job_lock_steps[0] < 0) return -1;
    out2[0] = bctx->job_lock_steps[0]; out2[1] = bctx->job_lock_steps[1];
    return 0;
}

static int copy_out(const std::vector<int32_t> & v, int per_row, int32_t * out, int capacity_rows) {
    const int rows = (int) v.size() / per_row;
    if (!out || capacity_rows < rows) return -1;
    if (rows) memcpy(out, v.data(), v.size() * 4);
    return rows;
}
int bark_hip_get_semantic_tokens(struct bark_context * bctx, int32_t * out, int capacity) { return bctx ? copy_out(bctx->semantic_tokens, 1, out, capacity) : -1; }
int bark_hip_get_coarse_tokens(struct bark_context * bctx, int32_t * out, int capacity_rows) { return bctx ? copy_out(bctx->coarse_tokens, 2, out, capacity_rows) : -1; }
int bark_hip_get_fine_tokens(struct bark_context * bctx, int32_t * out, int capacity_rows) { return bctx ? copy_out(bctx->fine_tokens, 8, out, capacity_rows) : -1; }

void bark_hip_get_stats(struct bark_context * bctx, struct bark_hip_stats * out) { if (bctx && out) *out = bctx->stats; }

double bark_hip_time_decode_step(struct bark_context * bctx, int which, int ctx, int iters, double * bytes_per_step) {
    if (!bctx) return -1.0;
    return guarded("bark_hip_time_decode_step", -1.0, [&] { return engine_time_decode_step(bctx, which, ctx, iters, bytes_per_step); });
}
double bark_hip_time_gemv(struct bark_context * bctx, int which, int op, int iters, double * bytes_per_launch) {
    if (!bctx) return -1.0;
    return guarded("bark_hip_time_gemv", -1.0, [&] { return engine_time_gemv(bctx, which, op, iters, bytes_per_launch); });
}
double bark_hip_time_fine_passes(struct bark_context * bctx, int n_windows, int iters, double * flops_per_pass) {
    if (!bctx) return -1.0;
    return guarded("bark_hip_time_fine_passes", -1.0, [&] { return engine_time_fine_pass(bctx, iters, flops_per_pass, n_windows); });
}

double bark_hip_time_fine_pass(struct bark_context * bctx, int iters, double * flops_per_pass) {
    if (!bctx) return -1.0;
    return guarded("bark_hip_time_fine_pass", -1.0, [&] { return engine_time_fine_pass(bctx, iters, flops_per_pass); });
}
double bark_hip_time_slots(struct bark_context * bctx, int which, int op, int n_slots, int kind, int ctx, int iters) {
    if (!bctx) return -1.0;
    return guarded("bark_hip_time_slots", -1.0, [&] { return engine_time_slots(bctx, which, op, n_slots, kind, ctx, iters); });
}
#ifdef BARK_TRACE
__attribute__((visibility("default"))) int bark_hip_trace_decode_step(struct bark_context * bctx, int which, int ctx, int replays, unsigned long long * out6, int cap_records) {
    if (!bctx || !out6) return -1;
    return guarded("bark_hip_trace_decode_step", -1, [&] { return engine_trace_decode_step(bctx, which, ctx, replays, out6, cap_records); });
}
#endif
const char * bark_hip_describe(struct bark_context * bctx) { return bctx ? bctx->description.c_str() : "no context"; }

}  // extern "C"
