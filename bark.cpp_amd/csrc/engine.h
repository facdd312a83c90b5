// engine.h - the MI355X Bark engine behind bark.h / bark_mi355x.h.
//
// Pipeline (reference call stack /root/reference/bark.cpp:2125-2172): tokenise -> semantic GPT ->
// coarse GPT (sliding windows) -> fine GPT (6 non-causal passes per window) -> EnCodec decoder.
// Weights live in one device slab; activations, KV caches and the per-stage StepState are
// device-resident; a decode step is a fixed kernel sequence captured once per model in a hipGraph
// and replayed per token with no host-side parameter updates.
#pragma once
#include "bark.h"
#include "bark_mi355x.h"
#include "kernels.h"
#include "model_file.h"
#include "tokenizer.h"

#include <functional>
#include <map>
#include <memory>
#include <random>
#include <string>
#include <vector>

struct bark_context;

namespace barkhip {

// ---- owners: each releases what it holds, so neither the context's destructor nor a throwing call lists handles ----
// A captured graph.  Move-only: state that holds one cannot be copied by accident (a clone captures its own).
struct GraphExec {
    GraphExec() = default;
    explicit GraphExec(hipGraphExec_t exec) : e(exec) {}
    GraphExec(GraphExec && o) noexcept : e(o.e) { o.e = nullptr; }
    GraphExec & operator=(GraphExec && o) noexcept { if (this != &o) { reset(); e = o.e; o.e = nullptr; } return *this; }
    ~GraphExec() { reset(); }
    void reset() { if (e) (void) hipGraphExecDestroy(e); e = nullptr; }
    explicit operator bool() const { return e != nullptr; }
    hipGraphExec_t get() const { return e; }
private:
    hipGraphExec_t e = nullptr;
};
// An event, created by its first record() (engine_internal.h).
struct Event {
    Event() = default;
    Event(Event && o) noexcept : e(o.e) { o.e = nullptr; }
    Event & operator=(Event && o) noexcept { if (this != &o) { reset(); e = o.e; o.e = nullptr; } return *this; }
    ~Event() { reset(); }
    void reset() { if (e) (void) hipEventDestroy(e); e = nullptr; }
    void record(hipStream_t s);
    hipEvent_t get() const { return e; }
private:
    hipEvent_t e = nullptr;
};
// Scratch that grows on demand: a VIEW of n elements at p.  The allocation belongs to the context (bark_context::allocs, as every dev_alloc), and one
// that a larger one has superseded stays there until the context is freed.  Trivially copyable: bark_context::Batch and HubScratch are copied by value.
template <typename T> struct DevBuf {
    T * p = nullptr; size_t n = 0;
    // a fresh allocation of exactly `count` elements, exactly when count > n (engine_internal.h).  Every buffer keeps its own n, so a group that grows
    // together (one reserve each, from one call) stays consistent when an allocation in the middle of it throws.
    void reserve(bark_context * ctx, size_t count);
};

// Immutable after load: clones copy it with a plain assignment and share the weights behind the pointers.
struct GptModel {
    GptHparams hp;
    const half_t * wte[8] = {};
    const half_t * lm_head[8] = {};
    // quantised model files (bark_model_quantize output): every weight matrix is a QMat instead of an f16 pointer
    bool q4 = false;                                    // activations stay f32 (quantised or f32 weights)
    bool w32 = false;                                   // f32 weights (QMat with qt == QT_F32)
    QMat wte_q[8], lm_head_q[8];
    const float * wpe = nullptr, * lnf_g = nullptr, * lnf_b = nullptr;
    struct Layer {
        const float * ln1_g = nullptr, * ln1_b = nullptr, * ln2_g = nullptr, * ln2_b = nullptr;
        const half_t * attn_w = nullptr, * proj_w = nullptr, * fc_w = nullptr, * mproj_w = nullptr;
        QMat attn_q, proj_q, fc_q, mproj_q;
        const float * attn_b = nullptr, * proj_b = nullptr, * fc_b = nullptr, * mproj_b = nullptr;
    };
    std::vector<Layer> layers;
    size_t kv_layer_stride = 0;                         // floats per layer of a KV cache of this model - the context's own (GptRun) or a batch slot's (0 for the
                                                        // fine model's shared scratch)
};
// What one context runs a GptModel with: its KV cache and its captured decode steps (bark_context::gpt_run, one per model)
struct GptRun {
    float * kcache = nullptr, * vcache = nullptr;       // [L][H][16][P][4] / [L][H][P][64] f32; fine model: L = 1 scratch
    float * vtcache = nullptr;                          // second copy of V in the K layout [L][H][16][P][4] (semantic / coarse): the decode attention
                                                        // reads 4 value dims of consecutive keys as one contiguous stream
    // layers -> LM head -> sample + embedding of the next token; [ng]: variant whose kernels request the keys below 256 ng without
    // waiting for the context length (the host knows how many rows the cache holds when it launches a step)
    GraphExec decode_graph[5];
    GraphExec decode_graph8[5];                         // eight such steps in one graph: one launch gap per eight tokens
    GraphExec bench_graph;                              // same, without advancing n_past (timing hook)
};

struct CodecModel {
    CodecHparams hp;
    int n_q = 0, D = 0;
    const float * codebooks = nullptr;                  // [n_q][n_bins][hidden_dim]
    // wm: kernel image for the matrix-core order C9m, [phases][cout32][kd16] f16 zero padded, kd = k * cin + ci (convT: one image per output
    // phase over tap * cin + ci), nullptr when cin is not a multiple of 8; w32: f32 copy of the file's kernel (exact) for order C9
    struct Conv { const half_t * w = nullptr; const float * w32 = nullptr; const float * b = nullptr; const half_t * wm = nullptr; int cout = 0, cin = 0, k = 0; };
    struct ConvT { const half_t * w = nullptr; const float * w32 = nullptr; const float * b = nullptr; const half_t * wm = nullptr; int cin = 0, cout = 0, k = 0, stride = 0; };
    struct Lstm { const half_t * w_ih = nullptr, * w_hh = nullptr; const float * b_ih = nullptr, * b_hh = nullptr; };
    Conv init, fin;
    Lstm lstm[2];
    struct Block { ConvT up; Conv c1, c2, sc; } blocks[4];
    // SEANet encoder (optional: files written without it report none).  Its tensors live in allocations of their own (SharedWeights::extra), so the
    // slab, its size and the decoder are what they are without an encoder.  down: the strided convolution behind the residual block (kernel 2 stride)
    struct EncBlock { Conv c1, c2, sc, down; int stride = 0; };
    struct Encoder { bool present = false; int F = 0; Conv init, fin; EncBlock blocks[4]; Lstm lstm[2]; } enc;
};

// The semantic encoder (rule C12h): HuBERT's feature encoder, projection, positional convolution and first `output_layer` layers, and
// the token head (two LSTM layers, a linear layer, argmax), loaded from a file of its own (bark_hip_load_semantic_encoder).  Immutable after load and held
// by shared pointer: the clones of a context share the device copy.
struct HubertModel {
    HubertHparams hp;
    int device = 0;
    std::vector<void *> bufs;                           // every device allocation of the model (freed with it)
    const half_t * conv0_w = nullptr; const float * gn_g = nullptr, * gn_b = nullptr; int k0 = 0;
    struct Conv { const half_t * wm = nullptr; const float * w32 = nullptr; int k = 0, stride = 0; } conv[6];      // C9m images [C32][kd16], kd = k C + ci
    const float * fp_ln_g = nullptr, * fp_ln_b = nullptr, * fp_b = nullptr; const half_t * fp_w = nullptr;
    const half_t * pos_w = nullptr; const float * pos_b = nullptr; int pos_co32 = 0, pos_kd = 0, pos_kd16 = 0;   // [G][co32][kd16], kd = k (H / G) + ci
    const float * enc_ln_g = nullptr, * enc_ln_b = nullptr;
    struct Layer {
        const half_t * qkv_w = nullptr, * o_w = nullptr, * fc1_w = nullptr, * fc2_w = nullptr;         // q, k and v rows stacked: [3 H][H]
        const float * qkv_b = nullptr, * o_b = nullptr, * fc1_b = nullptr, * fc2_b = nullptr, * ln1_g = nullptr, * ln1_b = nullptr, * ln2_g = nullptr, * ln2_b = nullptr;
    };
    std::vector<Layer> layers;
    CodecModel::Lstm lstm[2];
    const half_t * out_w = nullptr; const float * out_b = nullptr;
    const uint16_t * gelu_erf_lut = nullptr;            // f16(erf GELU(h)) for every f16 h: the FFN's epilogue (LinArgs::lut)
    HubertModel() = default;
    HubertModel(const HubertModel &) = delete;
    HubertModel & operator=(const HubertModel &) = delete;
    ~HubertModel();
};
constexpr int kHubMaxFrames = 1024;                     // T <= 1024: n <= 328 079 samples

// A voice prompt (rule C10v): the speaker history the three stage loops start from, copied from a bark_hip_voice_prompt.  Held
// by shared pointer: a context, the utterances of a job and the requests of a collector share one immutable copy.
struct VoicePrompt { std::vector<int32_t> semantic, coarse, fine; };      // [n_sem], [Tc][2], [Tf][8]
using VoicePtr = std::shared_ptr<const VoicePrompt>;

}  // namespace barkhip

// What the members of a context live in.  The base of bark_context, so it is destroyed after every member, which gives the release order of a context:
// ~bark_context selects the device, the members release their graphs and events (and, behind those, the last holder its share of the weights and the
// semantic encoder), then this frees the device allocations, the pinned host memory and, last, the stream.
struct bark_context_memory {
    int device = 0;
    hipStream_t stream = nullptr;
    std::vector<void *> allocs;                         // every dev_alloc: scratch, caches and what a grown DevBuf has left behind
    std::vector<void *> pinned;                         // every host_alloc
    bark_context_memory() = default;
    bark_context_memory(const bark_context_memory &) = delete;
    bark_context_memory & operator=(const bark_context_memory &) = delete;
    ~bark_context_memory();
};

// The opaque handle of bark.h.
struct bark_context : bark_context_memory {
    // What a context shares with its clones, immutable after load: the weight slab with the codec codebooks (bark_hip_clone_context: replicas on one
    // GPU stream the same bytes) and the semantic encoder.  Declared first, so the last context that holds them frees them behind its graphs and events.
    struct SharedWeights { void * slab = nullptr; void * codebooks = nullptr; std::vector<void *> extra; int device = 0; ~SharedWeights(); };
    std::shared_ptr<SharedWeights> weights;
    std::shared_ptr<const barkhip::HubertModel> hub;

    bark_context_params params;
    std::mt19937 rng;

    barkhip::Vocab vocab;
    barkhip::GptModel gpt[3];
    barkhip::GptRun gpt_run[3];
    barkhip::CodecModel codec;
    bool use_graph = true;
    // Order of the fine model's weight products on f16 model files.  0 (default policy): C1 - the restated reference order, on the
    // f32 matrix cores - for bark_generate_audio and the stage-level entry points, C1m - the f16 matrix cores' own accumulation - inside lock-step jobs
    // (in_job) and side-by-side fine passes; 1: C1 everywhere; 2: C1m everywhere (rounds 4 - 5).  BARK_HIP_FINE_ORDER=c1|c1m, bark_hip_set_fine_order.
    int fine_order = 0;
    bool in_job = false;                 // a lock-step job (engine_generate_batch) or a side-by-side fine pass is running on this context
    int fast_gemm = 0;                   // BARK_HIP_FAST_GEMM=1: N > 1 products on the f16 matrix cores in hardware accumulation order (non-canonical, tolerance mode)
    int decode_ng = 4;                                  // key groups (of 256) the decode kernels being enqueued may assume: ctx <= 256 ng

    size_t weight_bytes = 0;
    std::vector<std::pair<void *, size_t>> guarded;     // BARK_HIP_GUARD: {base of the allocation, bytes between its two guard bands}
    // GPT scratch
    float * x = nullptr, * q = nullptr, * logits = nullptr;
    float * knew = nullptr;                             // [E] K row appended by the current decode step (fixed-address copy)
    float * ps = nullptr;                               // [H][4][P] partial attention scores of a decode step (QKV kernel -> attn_ps_kernel)
    barkhip::half_t * xn = nullptr, * att = nullptr, * hbuf = nullptr;
    barkhip::half_t * q16 = nullptr, * k16 = nullptr, * vt16 = nullptr;      // tolerance route (fast_gemm): f16 operands of the flash attention, [P][E] each
    // quantised models: activations stay f32 between the products and are quantised to q8 rows (xq) in front of each
    bool any_q4 = false;
    float * att32 = nullptr, * h32 = nullptr; barkhip::Q8Scratch xq;
    bool any_w32 = false; float * xn32 = nullptr;       // f32 model files: LayerNorm-ed rows without f16 rounding
    int32_t * d_tokens = nullptr, * d_out_tokens = nullptr;
    float * d_eos_trace = nullptr;
    barkhip::StepState * d_state = nullptr;
    double * d_u = nullptr;                             // uniform draws for on-device multinomial sampling (8192)
    bool host_sampling = false;                         // BARK_HIP_HOST_SAMPLING=1: sample temp > 0 on the host (A/B path)
    // top-k / nucleus filter of the semantic and coarse samples (C8n, bark_hip_set_sampling_filter); {0, 1}: off.  The decode graphs read the
    // settings from d_filter (uploaded at the start of a stage), so only switching the filter on or off needs fresh graphs.
    bark_hip_sampling_filter filter{0, 1.0f};
    int32_t * d_filter = nullptr;                       // [0]: top_k, [1]: top_p (float bits)
    // speaker history of bark_generate_audio, the stage entry points and the jobs that carry no voices of their own (C10v, bark_hip_set_voice_prompt); null: none
    barkhip::VoicePtr voice;
    int32_t * d_fine_rel = nullptr;                     // [1] first position of the current fine window that keeps its pick (read by the captured pick kernels)
    uint16_t * d_gelu_lut = nullptr;
    int max_E = 0, max_H = 0, P = 1024;
    // codec scratch (grown on demand)
    barkhip::DevBuf<float> cbuf[3];                     // all six of one size
    barkhip::DevBuf<barkhip::half_t> cbuf_hh[3];
    barkhip::DevBuf<float> c_gi, c_cell, c_cell2; barkhip::DevBuf<barkhip::half_t> c_hseq_h, c_xt_h, c_hseq2_h;       // LSTM rows for c_gi.n / (4 D) frames; the cells
    barkhip::DevBuf<int32_t> d_codes;
    barkhip::GraphExec fine_graphs[16];                 // one captured forward pass + pick per predicted codebook, [8 * (products in C1m) + codebook]
    int * d_lstm_t = nullptr;                           // step counter of the replayed LSTM block
    barkhip::DevBuf<int> d_codec_T;                     // frame counts of the utterances being decoded and their prefix sums (CodecBatch)
    struct LstmGraph { barkhip::GraphExec exec; int B = 0; const float * out = nullptr; const float * gi = nullptr; } lstm_graph;    // 64 wave-front steps
    LstmGraph lstm_graph_enc;                           // the same block with the encoder's weights and row table: a slot of its own, so encode / decode never replay each other's capture
    barkhip::DevBuf<int> d_enc_T;                       // encoder: row counts and prefix sums of the recordings at each of its five stages ([5][80], laid out as d_codec_T)
    barkhip::DevBuf<float> d_pcm;                       // encoder: the recordings' samples back to back
    barkhip::Event enc_ev[2]; double enc_device_us = -1.0;      // events around the kernels of an encode call, and what the last call took between them
    const float * enc_latents = nullptr; int enc_latent_rows = 0;      // the latents [rows][hidden_dim] of the last encode call, until the next codec call of this context
    LstmGraph lstm_graph_hub;                           // ... and with the token head's (semantic encoder)
    // semantic encoder: this context's scratch for kHubMaxFrames frames (allocated with the first use)
    struct HubScratch {
        bool ready = false;
        float * pcm = nullptr; barkhip::half_t * pcm_h = nullptr;            // [n_max]
        barkhip::half_t * a16 = nullptr, * b16 = nullptr;                   // conv stack ping-pong: [T0_max][C], [T1_max][C]
        double * part = nullptr; float * stats = nullptr;                   // convolution 0: partial sums, statistics
        float * feat = nullptr;                                              // [T][C] end of the conv stack
        float * x = nullptr, * tmp = nullptr, * q = nullptr, * kc = nullptr, * vc = nullptr;     // [T][H] rows, K / V of one layer
        barkhip::half_t * xh = nullptr, * att = nullptr, * hb = nullptr;   // [T][max(C, H)], [T][H], [T][F]
        float * gi = nullptr, * c1 = nullptr, * c2 = nullptr, * out2 = nullptr; barkhip::half_t * h1 = nullptr, * h2 = nullptr;    // token head
        float * logits = nullptr; int32_t * ids = nullptr;                  // [T][n_classes], [T]
        int * rows = nullptr;                                                // [8][80] row tables of the conv stages (CodecBatch)
        barkhip::DevBuf<float> tap;                                          // parity tap 0 in f32 (grown on demand)
    } hubs;
    barkhip::Event hub_ev[2]; double hub_device_us = -1.0;
    barkhip::DevBuf<float> rs_in, rs_out;               // resampler (C13r): the recording and its 16 kHz form (grown on demand)
    // rational resampler (C14r): the taps of every pair used so far (uploaded once per pair), the segments' samples back to back, their results in the
    // requested format (both grown on demand) and the segment table [5][kResampleMaxSegments + 1]
    std::map<std::pair<int, int>, const float *> rp_taps;
    barkhip::DevBuf<float> rp_in; barkhip::DevBuf<uint8_t> rp_out; barkhip::DevBuf<int> rp_seg;
    // long-form join (C15j): the segment, activity and position tables of a call, the fade table of the last fade length used (jn_fade_F; -1: none yet)
    barkhip::DevBuf<int> jn_tab; barkhip::DevBuf<float> jn_fade; int jn_fade_F = -1;
    // speaking rate (C16t): the segments' samples back to back, their time-scaled 24 kHz form (what the resampler then reads in place of rp_in), the segment
    // table [6][kResampleMaxSegments + 1], the chosen positions (all grown on demand) and the window table (uploaded with the first use)
    barkhip::DevBuf<float> tp_in, tp_out, tp_win; barkhip::DevBuf<int> tp_seg, tp_pos; bool tp_win_ready = false;
    // loudness (C17l): the segments' samples back to back as given (the levelled ones go where the next stage reads: tp_in or rp_in), the segment table
    // [5][kResampleMaxSegments + 1], the z table, and one peak, request and info record per segment (the first three grown on demand)
    barkhip::DevBuf<float> lv_in; barkhip::DevBuf<int> lv_seg; barkhip::DevBuf<double> lv_z; barkhip::DevBuf<unsigned> lv_peak;
    barkhip::DevBuf<barkhip::LoudnessReq> lv_req; barkhip::DevBuf<barkhip::LoudnessInfo> lv_info;
    // FLAC (C18f): caller samples back to back (the routes encode where the format launch left its s16: rp_out), the segment table
    // [3][kResampleMaxSegments + 1], one slot of kFlacFrameStride bytes, a length and four ints per frame, the packed frames and [3][64] totals (grown on
    // demand); flac_lengths: the byte length of every stream the last conversion to BARK_HIP_SAMPLE_FLAC returned, in segment order
    barkhip::DevBuf<int16_t> fl_in; barkhip::DevBuf<int> fl_seg, fl_len, fl_info, fl_tot; barkhip::DevBuf<unsigned> fl_scratch; barkhip::DevBuf<uint8_t> fl_out;
    std::vector<int32_t> flac_lengths;
    struct CodecGraph { barkhip::GraphExec exec; std::vector<int> T; const float * buf = nullptr; float * out = nullptr; int tmul = 0; } codec_graph;   // conv stack behind the LSTM

    // batched decode (several utterances in lock step on this context, bark_hip_generate_batch): per-slot KV caches and decode rows,
    // the row scratch of the all-slots prefill; FineBatch below holds the scratch of the side-by-side fine passes
    struct Batch {
        int cap = 0;
        float * kc[2] = {nullptr, nullptr}, * vc[2] = {nullptr, nullptr}; size_t slot_stride[2] = {0, 0};
        float * x = nullptr, * q = nullptr, * logits = nullptr; barkhip::half_t * att = nullptr, * h = nullptr;
        barkhip::StepState * state = nullptr; int32_t * out_tokens = nullptr; float * eos_trace = nullptr; float * ln_stats = nullptr;
        float * att32 = nullptr, * h32 = nullptr;        // quantised models: f32 activations per slot
        float * sc = nullptr;                            // [cap][max_H][P] attention scores of a lock step (scores kernel -> mix kernel)
        float * ps = nullptr;                            // [cap][max_H][4][P] partial scores per slot (few-slot lock steps: QKV kernel -> attn_fused_ps_kernel)
        double * u = nullptr;                            // [cap][8192] uniform draws of the slots' own generators (temp > 0)
        size_t ld_logits = 0;
        float * slot_par = nullptr;                      // the slots' own temperatures [cap], min_eos_p [cap] (bark_hip_request_params) and top_p [cap]
        int32_t * slot_top_k = nullptr;                  // the slots' own top_k [cap] (bark_hip_sampling_filter)
        // pinned host memory (host_alloc): where the sampled ids [cap][2048] and the states [cap] of the live slots land at
        // a poll / window end, and the staging rows of the states uploaded at a window start
        int32_t * h_ids = nullptr; barkhip::StepState * h_state = nullptr, * h_state_in = nullptr;
        // window prompts of all slots in ONE pass (batch_prefill_many): row scratch for cap * P rows, the prompts' ids, the sequence table
        float * pf_x = nullptr, * pf_q = nullptr; barkhip::half_t * pf_xn = nullptr, * pf_att = nullptr, * pf_h = nullptr;
        int32_t * pf_tokens = nullptr; barkhip::SeqTab * pf_tab = nullptr;
    } batch;
    std::vector<float> h_slot_par;                      // host mirror of batch.slot_par
    std::vector<int32_t> h_slot_top_k;                  // host mirror of batch.slot_top_k
    struct StepMark { std::string name; barkhip::Event at; };
    std::vector<StepMark> * step_marks = nullptr;       // engine_profile_lock_step: events behind the launch sites of a lock step
    std::map<int, barkhip::GraphExec> batch_graphs;       // captured lock steps by (model, active slots, kinds of sampling among them)
    // fine windows of several utterances in one forward pass (engine_fine_many): rows = cap * 1024
    struct FineBatch {
        int cap = 0;
        float * x = nullptr, * q = nullptr, * logits = nullptr, * kc = nullptr, * vc = nullptr;
        barkhip::half_t * xn = nullptr, * att = nullptr, * hbuf = nullptr, * q16 = nullptr, * k16 = nullptr, * vt16 = nullptr;
        int32_t * tokens = nullptr, * rel = nullptr;     // [8][cap * 1024] window ids (codebook-major planes), [cap] first position of each window that keeps its pick
        double * u = nullptr;                            // [6][cap * 1024] uniform draws (fine_temp > 0)
    } fine_batch;
    struct BatchResult { std::vector<int32_t> semantic, coarse, fine; std::vector<float> audio; bool ok = false; };
    std::vector<BatchResult> batch_results;
    // the last bark_hip_generate_long call (C15s / C15j): the chunks' spans in the text, their results (untrimmed) and the join parameters; no chunk: none held
    // joined / layout: what the last bark_hip_long_audio_as made, in joined_fmt (sample_rate 0: nothing yet), so that a probe for the size and the call that
    // fetches the bytes join once
    struct LongResult {
        std::vector<barkhip::TextSpan> spans; std::vector<BatchResult> chunks; bark_hip_join_params join{6000, 0, 0.0f, 0};
        std::vector<uint8_t> joined; std::vector<int32_t> layout; bark_hip_audio_format joined_fmt{0, 0};
        int joined_speed = 1000;                         // the speed `joined` was made at (bark_hip_long_audio_at); layout is always that of speed 1000
        bark_hip_loudness_params joined_loudness{0, 0.0f, 0.0f};      // and the levelling (bark_hip_long_audio_with; target 0: none)
        std::vector<bark_hip_loudness_info> joined_info;               // one record per chunk of that levelling
    } long_result;
    // lock steps (batch_step calls) of the last bark_hip_generate_batch job: [0] semantic stage, [1] coarse stage; {0, 0}: the sequential fallback took
    // the job; -1: no job has run (bark_hip_batch_lock_steps)
    int32_t job_lock_steps[2] = {-1, -1};
    bark_context * tail = nullptr;                      // clone that runs the fine passes / codec of a lock-step job beside its decode chain (engine_batch.hip: JobTail)

#ifdef BARK_TRACE
    unsigned long long * trace_rec = nullptr; unsigned * trace_pos = nullptr; unsigned trace_cap = 0; int trace_kid = 0; unsigned trace_base = 0, trace_per_replay = 0;
#endif
    // results of the last generate call
    std::vector<int32_t> tokens, semantic_tokens, coarse_tokens, fine_tokens;
    std::vector<float> audio;
    std::vector<float> eos_trace;
    bark_hip_stats stats{};
    std::string description;

    ~bark_context();
};

namespace barkhip {

// All functions throw std::runtime_error on failure; the C API catches at the boundary.
bark_context * engine_load(const char * path, const bark_context_params & params, uint32_t seed, int device = -1);      // device < 0: BARK_HIP_DEVICE / the current device
bark_context * engine_clone(bark_context * src, uint32_t seed);          // same weights, own stream / caches / scratch
void engine_invalidate_graphs(bark_context * ctx);

int  engine_gpt_eval(bark_context * ctx, int which, const int32_t * tokens, int n_tokens, int n_past, bool merge_ctx, float * logits);
void engine_fine_eval(bark_context * ctx, const int32_t * tokens_8x1024, int nn, float * logits);

std::vector<int32_t> engine_semantic(bark_context * ctx, const std::vector<int32_t> & prompt, std::vector<float> * eos_trace);
// coarse and fine start from the context's voice prompt, if it has one (C10v); both return the NEW frames only
std::vector<int32_t> engine_coarse(bark_context * ctx, const std::vector<int32_t> & semantic);          // [T][2]
std::vector<int32_t> engine_fine(bark_context * ctx, const std::vector<int32_t> & coarse_Tx2);          // [T][8]
// the fine stage of several utterances, their windows side by side in every forward pass (f16 model files; per-utterance results are those
// of engine_fine); rngs: one generator per utterance (fine_temp > 0), advanced as engine_fine advances the context's; voices: one voice prompt
// per utterance (entries may be null: no voice), nullptr: the context's for everyone
std::vector<std::vector<int32_t>> engine_fine_many(bark_context * ctx, const std::vector<const std::vector<int32_t> *> & coarse, std::vector<std::mt19937> * rngs,
                                                   const std::vector<const VoicePrompt *> * voices = nullptr);
// checks a voice prompt against the context's parameters and models (ids in range, non-empty trimmed history, history + first coarse window within the
// coarse context) and copies it; throws on a bad one.  v == nullptr: a null pointer (no voice)
VoicePtr engine_make_voice(const bark_context * ctx, const bark_hip_voice_prompt * v);
// ids 256..511 of a 513-id semantic prompt <- the last min(n_sem, 256) history ids, right-padded with semantic_pad_token (C10v.1)
void engine_voice_into_prompt(const bark_context_params & p, const VoicePrompt * v, std::vector<int32_t> & prompt513);
// kernel-level hook (tests): the fine stage's pick launches on caller rows - n_windows * 1024 rows of n_cols logits, temp == 0: argmax_rows, else
// sample_rows_multinomial with u[row]; tokens_io [n_windows * 1024] holds the plane before and after (row z * 1024 + j is written when j >= rel[z])
void engine_pick_rows(bark_context * ctx, const float * logits, int n_windows, int n_cols, float temp, const double * u, const int32_t * rel, int32_t * tokens_io,
                      int32_t * near_ties);
// tap_stage >= 0: *tap receives the activation after that stage (0 first conv, 1 LSTM+skip, 2..5 up-blocks)
std::vector<float>   engine_codec_decode(bark_context * ctx, const int32_t * codes, int n_q, int T, int tap_stage, std::vector<float> * tap);
// all utterances of a batch in one pass (codes[b]: [n_q][T[b]]); the launches of one utterance serve all of them
std::vector<std::vector<float>> engine_codec_decode_many(bark_context * ctx, const std::vector<const int32_t *> & codes, int n_q, const std::vector<int> & T,
                                                         int tap_stage, std::vector<float> * tap);
// EnCodec encoder: n <= 32 recordings (pcm[b]: n_samples[b] floats, 24 kHz mono) in one pass -> codes[b] [n_q][T[b]], T[b] = ceil(n_samples[b] / 320).
// tap_stage >= 0 (one recording): *tap receives the activation after that stage, channel-major (0 first conv, 1..4 the down-sampling convs, 5 LSTM + skip,
// 6 the latent [H][T]).  Throws without an encoder in the file, on an empty / too long (> 4096 frames) / non-finite recording, on n_q outside the file's codebooks.
std::vector<std::vector<int32_t>> engine_codec_encode_many(bark_context * ctx, const std::vector<const float *> & pcm, const std::vector<int> & n_samples, int n_q,
                                                           int tap_stage, std::vector<float> * tap);
// Semantic encoder (C12h).  engine_load_semantic_encoder: parse, check and upload the file (throws on a malformed / quantised / mis-shaped one); the context
// and every clone made afterwards share it.  engine_semantic_encode: n samples of 16 kHz mono -> T = (n - 400) / 320 + 1 ids; tap_stage >= 0: *tap receives that
// stage's rows (0 conv 0 [T0][C], 1 conv stack [T][C], 2 projection [T][H], 3 hidden_states[0], 4 hidden_states[L], 5 logits [T][n_classes]).  engine_semantic_head:
// the token head alone on caller rows [T][H]
void engine_load_semantic_encoder(bark_context * ctx, const char * path);
std::vector<int32_t> engine_semantic_encode(bark_context * ctx, const float * pcm16k, int n, int tap_stage, std::vector<float> * tap);
std::vector<int32_t> engine_semantic_head(bark_context * ctx, const float * feats_TxH, int T, std::vector<float> * logits);
// Resampler (C13r): n samples at 24 kHz (1 .. 4096 codec frames, all finite) -> (2 n + 2) / 3 samples at 16 kHz.  engine_voice_from_audio: the whole voice prompt
// of a recording - its last kVoiceAudioMaxSamples samples through the resampler and the semantic encoder, and through the codec encoder (8 codebooks; the
// first two are the coarse stream) - checked as engine_make_voice checks one; throws where any of the steps or that check refuses.
constexpr int kVoiceAudioMaxSamples = 480000;
std::vector<float> engine_resample_24k_16k(bark_context * ctx, const float * pcm24k, int n);
VoicePtr engine_voice_from_audio(bark_context * ctx, const float * pcm24k, int n);
double engine_time_resample(bark_context * ctx, int n, int iters);
// Rational resampler and sample formats (C14r).  Rates: 8000, 12000, 16000, 22050, 24000, 32000, 44100, 48000 with 24000 on at least one side;
// rate_in == rate_out (24000) is the identity.  resample_pair_table: L, M, half and the taps [L][2 half] of a pair, computed once per process in double
// precision and rounded to f32 (24000 -> 16000: the committed table of C13r); nullptr for the identity and for an unsupported pair.
// resample_out_len: ceil(n L / M), n for the identity, -1 for an unsupported pair or n < 0.
struct ResampleTable { int L = 1, M = 1, half = 1; std::vector<float> h; };
const ResampleTable * resample_pair_table(int rate_in, int rate_out);
bool resample_pair_supported(int rate_in, int rate_out);
long long resample_out_len(long long n, int rate_in, int rate_out);
inline int sample_format_bytes(int fmt) { return fmt == BARK_HIP_SAMPLE_F32 ? 4 : fmt == BARK_HIP_SAMPLE_S16 ? 2 : fmt == BARK_HIP_SAMPLE_MULAW ? 1 : 0; }
// BARK_HIP_SAMPLE_FLAC (rule C18f) is a container over the s16 samples: the format launches write pcm_format(fmt), and the calls that render a held result
// (engine_resample_many, _tempo_many, _level_many, _join_many) then encode where those samples lie and return the streams back to back, their byte lengths
// in ctx->flac_lengths.  sample_format_bytes stays 0 for it: a call that has not been taught the container refuses it.
inline int pcm_format(int fmt) { return fmt == BARK_HIP_SAMPLE_FLAC ? BARK_HIP_SAMPLE_S16 : fmt; }
inline int render_format_bytes(int fmt) { return sample_format_bytes(pcm_format(fmt)); }
// count <= 64 segments (1 .. 1 310 720 finite samples each) in ONE launch -> their results back to back as bytes of the format, n_out[i] samples each;
// bit-identical to count single calls.  Throws on a bad count / length / sample / pair / format.
std::vector<uint8_t> engine_resample_many(bark_context * ctx, const float * const * pcm, const int * n, int count, int rate_in, int rate_out, int fmt,
                                          std::vector<int32_t> & n_out);
double engine_time_resample_pair(bark_context * ctx, int n, int rate_in, int rate_out, int fmt, int iters);
// Long-form join (C15j): count <= 64 segments of 24 kHz f32 (1 .. 1 310 720 finite samples each) -> trim by frame activity, fade, gaps of +0 between
// the non-empty kept ranges, then format(C14r(J, 24000 -> rate_out)) of the joined signal J (N <= 2^25 samples; N == 0: no bytes) - at most two launches
// whatever the count (threshold 0: the host writes the activity table, one launch).  layout [count][2]: first sample in J and kept samples of every segment.  Throws on a bad count / length / sample / parameter /
// rate / format and on N > 2^25.  join_params_valid: gap >= 0, fade 0 .. 24000, threshold >= 0 and finite, pad >= 0.
inline bark_hip_join_params join_default_params() { return bark_hip_join_params{6000, 0, 0.0f, 0}; }
bool join_params_valid(const bark_hip_join_params & p);
std::vector<uint8_t> engine_join_many(bark_context * ctx, const float * const * pcm, const int * n, int count, const bark_hip_join_params & p, int rate_out, int fmt,
                                      std::vector<int32_t> & layout);
// the layout alone: the checks and the active frames (one launch with a threshold, none without), no sample staged or filtered
std::vector<int32_t> engine_join_layout(bark_context * ctx, const float * const * pcm, const int * n, int count, const bark_hip_join_params & p);
// device time of the join launch (all a default call runs: threshold 0 needs no activity launch) or, activity: of the table's fill + the activity launch alone
double engine_time_join(bark_context * ctx, int count, int n_each, int rate_out, int fmt, int iters, bool activity = false);
// Speaking rate (C16t): count <= 64 segments of 24 kHz f32 (1 .. 1 310 720 finite samples each, |x| < 65520), a speed per segment in per mille (500 .. 2000;
// 1000: the identity) -> format(C14r(C16t(x), 24000 -> rate_out)), the segments' results back to back: one tempo launch (none if every speed is 1000), then
// what engine_resample_many runs, reading the time-scaled samples where they lie on the device.  n_out: samples per segment at rate_out.  positions (may
// be null): the frames' chosen positions, K = ceil(ceil(1000 n / p) / 360) per segment back to back.  Throws on a refusal.  tempo_out_len: ceil(1000 n / p),
// or -1 (n outside 1 .. 1 310 720, p outside 500 .. 2000).
long long tempo_out_len(long long n, int speed_permille);
std::vector<uint8_t> engine_tempo_many(bark_context * ctx, const float * const * pcm, const int * n, int count, const int32_t * speed_permille, int rate_out, int fmt,
                                       std::vector<int32_t> & n_out, std::vector<int32_t> * positions = nullptr);
double engine_time_tempo(bark_context * ctx, int count, int n_each, int speed_permille, int iters);
// Loudness (C17l): count <= 64 segments of 24 kHz f32 under the tempo calls' limits, a request per segment (target_centilufs 0: off - measured, gain 1).
// loudness_params_valid: target 0 or -4000 .. -500, ceiling and cap >= 0 and finite.  loudness_target_ms: 10^((t / 100 + 0.691) / 10) in double.
// engine_loudness_many: the two launches without the scaled copy (params may be null: every gain 1); z (may be null): the hop tables back to back.
// engine_level_many: the two launches, the levelled samples written where the next stage reads them, then what engine_tempo_many runs behind its upload
// (the tempo launch if a speed is not 1000, the resampler / format launches) - nothing returns to the host in between.  Every request off: the call IS
// engine_tempo_many and info is {gain 1, all else 0}.  Both throw on a refusal.
bool loudness_params_valid(const bark_hip_loudness_params & p);
double loudness_target_ms(int target_centilufs);
std::vector<bark_hip_loudness_info> engine_loudness_many(bark_context * ctx, const float * const * pcm, const int * n, int count, const bark_hip_loudness_params * params,
                                                         std::vector<double> * z = nullptr);
std::vector<uint8_t> engine_level_many(bark_context * ctx, const float * const * pcm, const int * n, int count, const bark_hip_loudness_params * params,
                                       const int32_t * speed_permille, int rate_out, int fmt, std::vector<int32_t> & n_out, std::vector<bark_hip_loudness_info> * info = nullptr);
// FLAC (C18f): count <= 64 results of 1 .. 2^26 mono s16 samples at one of the eight rates -> their streams (marker, STREAMINFO, frames) back to back, in the
// two launches whatever the count; lengths: bytes per stream; frames (may be null): {subframe code, partition order, byte length, CRC-16} per frame, the
// results' frames back to back.  Only the packed frames, the totals and (if asked for) the frame records return to the host, which writes the 42 bytes in
// front of every stream.  Throws on a refusal.  flac_max_bytes: 42 + 14 ceil(n / 4096) + 2 n, or -1 for n outside 1 .. 2^26.
long long flac_max_bytes(long long n);
std::vector<uint8_t> engine_flac_encode_many(bark_context * ctx, const int16_t * const * pcm, const int * n, int count, int rate, std::vector<int32_t> & lengths,
                                             std::vector<int32_t> * frames = nullptr);
// device time of ONE pair of launches (which 0), ONE frames launch (1) or ONE pack launch (2) over `count` results of n_each samples of a synthetic voiced
// signal at 24 kHz
double engine_time_flac(bark_context * ctx, int count, int n_each, int iters, int which = 0);
// device time of ONE loudness_hops launch (level false) or ONE loudness_level launch with its scaled copy (level true) over `count` segments of n_each samples
double engine_time_loudness(bark_context * ctx, int count, int n_each, int iters, bool level);
// Long-form text (C15s + C15j): split, run the chunks (chain 0: ONE lock-step job, chunk i with seed rp.seed + i; chain 1: one job per chunk, chunk
// i + 1 with the voice made of chunk i's three streams, the previous voice where that one is refused), keep the results in ctx->long_result.  Returns
// the chunk count; throws if a chunk fails.  A text without a word runs as one chunk.
int engine_generate_long(bark_context * ctx, const char * text, const bark_hip_long_params & lp, const bark_hip_request_params * rp, const bark_hip_sampling_filter * flt,
                         const VoicePtr * voice);
// kernel-level hook: latents [T][H] -> codes [n_q][T] by the RVQ kernel alone (C11q)
std::vector<int32_t> engine_rvq_encode(bark_context * ctx, const float * latents, int T, int n_q);
bool engine_generate(bark_context * ctx, const char * text);
// seeds: one std::mt19937 seed per utterance (temp > 0); nullptr: drawn from the context's generator, in order.  Returns #ok
// Continuous admission: while the semantic stage of a job has free slots and nobody of the job waits for them, next() may hand over further
// requests (false: none pending); they join the job - results are appended behind the n given ones - up to max_job utterances in total.
struct BatchAdmit { std::function<bool(std::string & text, bark_hip_request_params & rp, bark_hip_sampling_filter & flt, VoicePtr & voice)> next; int max_job = 0; };
// rps: per-utterance parameters (nullptr: the context's for everyone); seeds override rps[i].seed when both are given;
// flts: per-utterance top-k / nucleus filters (nullptr: the context's for everyone); voices: per-utterance voice prompts (nullptr, or a null entry:
// the context's)
int  engine_generate_batch(bark_context * ctx, const char * const * texts, int n, const uint32_t * seeds, const bark_hip_request_params * rps = nullptr,
                           const BatchAdmit * admit = nullptr, const bark_hip_sampling_filter * flts = nullptr, const VoicePtr * voices = nullptr);
// checks a filter (top_k >= 0, 0 < top_p <= 1); false on a bad one
bool filter_valid(const bark_hip_sampling_filter & f);
inline bool filter_on(const bark_hip_sampling_filter & f) { return f.top_k > 0 || f.top_p < 1.0f; }
// the decode loop's filter + sampler launches on n_rows caller rows of n logits (bark_hip_sample_rows_filtered): ids, eos_p = p_{n-1}
void engine_sample_rows_filtered(bark_context * ctx, const float * logits, int n_rows, int n, const float * temp, const int32_t * top_k, const float * top_p,
                                 const double * u, int32_t * out_ids, float * out_eos_p);
// the same launches with per-row stop thresholds and stage states, per-call mode / eos token / slice base / prescaled / n_past_add, and optionally
// one single-slot launch per row (bark_hip_sample_rows_state); state_io: eight int32 per row, before the launch in, after it out
void engine_sample_rows_state(bark_context * ctx, const float * logits, int n_rows, int n, const float * temp, const int32_t * top_k, const float * top_p,
                              const double * u, const float * min_eos_p, const bark_hip_sample_call & call, int32_t * state_io, int32_t * out_ids,
                              float * out_eos_p);
double engine_time_sample_filtered(bark_context * ctx, int n, int n_rows, int top_k, float top_p, int peaked, int iters);
void engine_reserve_batch(bark_context * ctx, int slots);          // fixes the lock-step capacity (otherwise the first batch call does)

double engine_time_decode_step(bark_context * ctx, int which, int ctxlen, int iters, double * bytes_per_step);
double engine_time_gemv(bark_context * ctx, int which, int op, int iters, double * bytes_per_launch);
double engine_time_fine_pass(bark_context * ctx, int iters, double * flops_per_pass, int Z = 1);     // Z windows side by side (engine_fine_many's pass)
double engine_time_slots(bark_context * c, int which, int op, int B, int kind, int ctxlen, int iters);
void engine_profile_lock_step(bark_context * c, int which, int B, int ctxlen, int reps, std::vector<std::pair<std::string, double>> & out);
#ifdef BARK_TRACE
int engine_trace_decode_step(bark_context * ctx, int which, int ctxlen, int replays, unsigned long long * out6, int cap_records);
#endif

}  // namespace barkhip
