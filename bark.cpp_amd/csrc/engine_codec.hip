// engine_codec.hip - EnCodec decode and encode (decode: encodec_decompress_audio call site, /root/reference/bark.cpp:2143-2167) for one utterance or
// for all utterances of a lock-step batch at once.  Architecture: HF modeling_encodec.py:316-347 (decoder stack), :236-249 (LSTM +
// skip), :252-282 (residual blocks), :381-448 (RVQ de-embedding); kernels in codec_kernels.hip, the LSTM input projection in kernels.hip.
#include "engine_internal.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <stdexcept>

using namespace barkhip;
using namespace barkhip::detail;


namespace {
// scratch shared by decode and encode: three f32 and three f16 activation buffers of `need` elements, the LSTM's rows for Ts frames, its cells, the row tables
void ensure_codec_scratch(bark_context * c, size_t need, int Ts, int D) {
    for (auto & b : c->cbuf) b.reserve(c, need);
    for (auto & b : c->cbuf_hh) b.reserve(c, need);
    const size_t rows = (size_t) Ts * D;                         // D is the model's: the four grow together
    c->c_gi.reserve(c, 4 * rows); c->c_hseq_h.reserve(c, rows); c->c_xt_h.reserve(c, rows); c->c_hseq2_h.reserve(c, rows);
    c->c_cell.reserve(c, (size_t) 32 * D); c->c_cell2.reserve(c, (size_t) 32 * D); c->d_codec_T.reserve(c, 80);
}

// 2-layer LSTM (modeling_encodec.py:236-249) over the f16 rows c->c_xt_h [Ts][D] -> out2 [Ts][D] f32 (the skip is the caller's), both layers as a wave
// front: launch i = layer 1 at step i + layer 2 at step i - 1 (its input projection formed in the same kernel): T + 1 strictly sequential launches
// instead of 2 T, for all utterances at once.  64 of them are captured once as a hipGraph whose nodes take their launch index from a device counter,
// so one graph serves every T (and is re-captured only when the batch size or a buffer changes).  `slot`: the capture of THESE weights and THIS row
// table (decoder and encoder each own one).
// `io`: the rows and state buffers (the codec's own by default); the semantic encoder's token head brings its own, and an input width K_in != D
struct LstmIo { const half_t * x_h; int K_in, D; float * gi, * c1, * c2; half_t * h1, * h2; };
LstmIo codec_lstm_io(bark_context * c) { return LstmIo{c->c_xt_h.p, c->codec.D, c->codec.D, c->c_gi.p, c->c_cell.p, c->c_cell2.p, c->c_hseq_h.p, c->c_hseq2_h.p}; }
void run_lstm_pair(bark_context * c, const CodecModel::Lstm * lstm, bark_context::LstmGraph & slot, const CodecBatch & cb, int Ts, int Tmax, float * out2, const LstmIo & io) {
    hipStream_t s = c->stream;
    const int D = io.D, B = cb.B;
    {
        LinArgs g;
        g.W = lstm[0].w_ih; g.M = 4 * D; g.K = io.K_in; g.N = Ts; g.x_f16 = io.x_h; g.epi = EPI_LOGITS; g.out = io.gi; g.ld_out = 4 * D;
        launch_linear(s, g);
    }
    LstmPairArgs a;
    a.gi1 = io.gi; a.w_hh1 = lstm[0].w_hh; a.b_ih1 = lstm[0].b_ih; a.b_hh1 = lstm[0].b_hh; a.c1 = io.c1; a.h1 = io.h1;
    a.w_ih2 = lstm[1].w_ih; a.w_hh2 = lstm[1].w_hh; a.b_ih2 = lstm[1].b_ih; a.b_hh2 = lstm[1].b_hh; a.c2 = io.c2; a.h2 = io.h2;
    a.out2 = out2; a.T = Tmax; a.D = D; a.cb = cb;
    if (!c->use_graph) {
        for (int i = 0; i <= Tmax; i++) { a.t = i; launch_lstm_pair_step(s, a); }
        return;
    }
    constexpr int kBlock = 64;
    if (slot.out != out2 || slot.gi != io.gi || slot.B != B) slot.exec.reset();
    if (!slot.exec) {
        slot.exec = capture_graph(s, [&] {
            a.t_base = c->d_lstm_t;
            for (int i = 0; i < kBlock; i++) { a.t = i; launch_lstm_pair_step(s, a); }
            launch_add_int(s, c->d_lstm_t, kBlock);
        });
        slot.out = out2; slot.gi = io.gi; slot.B = B;
    }
    const int hdr[2] = {0, Tmax};
    HIP_OK(hipMemcpyAsync(c->d_lstm_t, hdr, sizeof(hdr), hipMemcpyHostToDevice, s));
    HIP_OK(hipStreamSynchronize(s));                         // hdr is a stack object
    for (int i0 = 0; i0 <= Tmax; i0 += kBlock) HIP_OK(hipGraphLaunch(slot.exec.get(), s));
}

// C11q: rvq_encode_kernel writes -1 for a frame in which no distance compared below +inf (a non-finite latent): an error, never a code
void throw_on_missing_pick(const std::vector<int32_t> & codes) {
    for (int32_t v : codes) if (v < 0) throw std::runtime_error("codec: a latent frame has no finite distance to any codebook row (non-finite latent)");
}
}  // namespace

namespace barkhip {

// codes[b]: [n_q][T[b]] ids of utterance b.  Every activation is time-major [row][C] with the utterances' rows back to back (CodecBatch,
// kernels.h): one launch per operator for the whole batch, the T + 1 strictly sequential LSTM launches of an utterance shared by all.
// tap_stage >= 0 (one utterance only): *tap receives the activation after that stage (0 first conv, 1 LSTM + skip, 2..5 up-blocks).
std::vector<std::vector<float>> engine_codec_decode_many(bark_context * c, const std::vector<const int32_t *> & codes, int n_q, const std::vector<int> & T,
                                                         int tap_stage, std::vector<float> * tap) {
    HIP_OK(hipSetDevice(c->device));
    c->enc_latents = nullptr; c->enc_latent_rows = 0;
    CodecModel & cm = c->codec;
    const int B = (int) T.size();
    if (B < 1 || B > 32 || codes.size() != T.size()) throw std::runtime_error("codec: 1..32 utterances per call");
    if (tap_stage >= 0 && B != 1) throw std::runtime_error("codec: activation taps take one utterance");
    if (n_q <= 0 || n_q > cm.n_q) throw std::runtime_error("codec: bad code matrix shape");
    std::vector<int> Tpre((size_t) B + 1, 0);
    int Tmax = 0;
    for (int b = 0; b < B; b++) {
        if (T[(size_t) b] <= 0 || T[(size_t) b] > 4096) throw std::runtime_error("codec: bad code matrix shape");
        for (size_t i = 0; i < (size_t) n_q * T[(size_t) b]; i++) if (codes[(size_t) b][i] < 0 || codes[(size_t) b][i] >= cm.hp.n_bins) throw std::runtime_error("codec: code out of range");
        Tpre[(size_t) b + 1] = Tpre[(size_t) b] + T[(size_t) b];
        Tmax = std::max(Tmax, T[(size_t) b]);
    }
    const int Ts = Tpre[(size_t) B];                              // frames of the whole batch
    hipStream_t s = c->stream;
    const int D = cm.D;
    // largest activation: rows x channels at every stage (time-major; the hidden channels of a residual block are half its width)
    size_t need = (size_t) std::max(cm.hp.hidden_dim, D) * Ts;
    { int ch = D; size_t tt = (size_t) Ts; for (auto & b : cm.blocks) { ch = b.up.cout; tt *= b.up.stride; need = std::max(need, (size_t) ch * tt); } }
    ensure_codec_scratch(c, need, Ts, D);
    c->d_codes.reserve(c, (size_t) n_q * Ts);
    for (int b = 0; b < B; b++)
        HIP_OK(hipMemcpyAsync(c->d_codes.p + (size_t) n_q * Tpre[(size_t) b], codes[(size_t) b], (size_t) n_q * T[(size_t) b] * 4, hipMemcpyHostToDevice, s));
    // device copies of the frame counts and their prefix sums: [0, 32) T, [40, 73) Tpre
    {
        int hdr[80] = {};
        for (int b = 0; b < B; b++) hdr[b] = T[(size_t) b];
        for (int b = 0; b <= B; b++) hdr[40 + b] = Tpre[(size_t) b];
        HIP_OK(hipMemcpyAsync(c->d_codec_T.p, hdr, sizeof(hdr), hipMemcpyHostToDevice, s));
        HIP_OK(hipStreamSynchronize(s));                        // hdr is a stack object
    }
    CodecBatch cb; cb.T = c->d_codec_T.p; cb.Tpre = c->d_codec_T.p + 40; cb.B = B;
    // time-major buffers: three f32 (A / Bf / R) and three f16 (H0 / H1 / H2)
    float * A = c->cbuf[0].p, * Bf = c->cbuf[1].p, * R = c->cbuf[2].p;
    half_t * H0 = c->cbuf_hh[0].p, * H1 = c->cbuf_hh[1].p, * H2 = c->cbuf_hh[2].p;

    // one convolution over time-major rows: xh [rows_in][cin] f16 -> any of y (f32), yh_raw, yh_elu (f16: what the next operators consume)
    auto conv_args = [&](const half_t * wm, const float * w32, const float * bias, int cin, int cout, int K, int stride, const half_t * xh, int tm_in) {
        ConvTmArgs a;
        a.W = wm; a.w32 = w32; a.bias = bias; a.cin = cin; a.cout = cout; a.cout32 = (cout + 31) & ~31; a.K = K;
        a.convT = stride > 0 ? 1 : 0; a.nphase = stride > 0 ? stride : 1;
        a.kd = (stride > 0 ? 2 : K) * cin; a.kd16 = (a.kd + 15) & ~15;
        a.xh = xh; a.rows_in = Ts * tm_in; a.tm_in = tm_in; a.cb = cb;
        return a;
    };
    auto conv = [&](const CodecModel::Conv & cv, const half_t * xh, int tm, const float * add, float * y, half_t * yh_raw, half_t * yh_elu) {
        ConvTmArgs a = conv_args(cv.wm, cv.w32, cv.b, cv.cin, cv.cout, cv.k, 0, xh, tm);
        a.add = add; a.y = y; a.yh_raw = yh_raw; a.yh_elu = yh_elu;
        launch_conv_tm(s, a);
    };
    // RVQ de-embedding, first conv
    launch_rvq_gather(s, cm.codebooks, cm.hp.n_bins, cm.hp.hidden_dim, c->d_codes.p, n_q, Tmax, Ts, A, cb);
    launch_act_round(s, A, (size_t) cm.hp.hidden_dim * Ts, 0, H0);
    conv(cm.init, H0, 1, nullptr, Bf, c->c_xt_h.p, nullptr);      // Bf = x [row][D]; its f16 image is the LSTM's input
    run_lstm_pair(c, cm.lstm, c->lstm_graph, cb, Ts, Tmax, R, codec_lstm_io(c));
    // parity taps are handed out channel-major [C][T'] (one utterance)
    auto grab = [&](int stage, const float * buf, int C, size_t rows) {
        if (tap_stage != stage || !tap) return;
        std::vector<float> tm((size_t) C * rows);
        HIP_OK(hipMemcpyAsync(tm.data(), buf, tm.size() * 4, hipMemcpyDeviceToHost, s));
        HIP_OK(hipStreamSynchronize(s));
        tap->resize(tm.size());
        for (size_t r = 0; r < rows; r++) for (int ch = 0; ch < C; ch++) (*tap)[(size_t) ch * rows + r] = tm[r * (size_t) C + ch];
    };
    grab(0, Bf, D, (size_t) Ts);
    // skip connection + the four upsampling blocks + final conv: ~25 launches, replayed from a hipGraph captured per list of frame
    // counts (the buffers are the context's own, so a graph stays valid until they are re-allocated for a longer input)
    int tmul = 1;
    float * pcm_dev = nullptr;
    auto tail = [&](bool taps) {
        launch_add(s, R, Bf, (size_t) D * Ts, A);                    // y + x
        if (taps) grab(1, A, D, (size_t) Ts);
        launch_act_round(s, A, (size_t) D * Ts, 1, H0);             // H0 = f16(ELU(x))
        tmul = 1;
        for (int b = 0; b < 4; b++) {
            const CodecModel::Block & bl = cm.blocks[b];
            // upsampling of f16(ELU(x)) (H0): the next operators consume only the f16 images of its result - as it is (shortcut input, H1) and
            // after the ELU (conv1 input, H2)
            ConvTmArgs u = conv_args(bl.up.wm, bl.up.w32, bl.up.b, bl.up.cin, bl.up.cout, bl.up.k, bl.up.stride, H0, tmul);
            u.yh_raw = H1; u.yh_elu = H2;
            launch_conv_tm(s, u);
            tmul *= bl.up.stride;
            // residual block: shortcut(x) + conv2(elu(conv1(elu(x))))   (modeling_encodec.py:252-282)
            conv(bl.c1, H2, tmul, nullptr, nullptr, nullptr, H0);           // H0 = f16(ELU(conv1(...)))
            conv(bl.c2, H0, tmul, nullptr, R, nullptr, nullptr);            // R = r (f32: it is added, not multiplied)
            conv(bl.sc, H1, tmul, R, taps ? A : nullptr, nullptr, H0);      // shortcut(x) + r; H0 = f16(ELU(..)): the next block's / the last conv's input
            if (taps) grab(2 + b, A, bl.up.cout, (size_t) Ts * tmul);
        }
        conv(cm.fin, H0, tmul, nullptr, Bf, nullptr, nullptr);
        pcm_dev = Bf;
    };
    if (c->use_graph && tap_stage < 0) {
        auto & cg = c->codec_graph;
        if (cg.T != T || cg.buf != A) cg.exec.reset();
        if (!cg.exec) {
            cg.exec = capture_graph(s, [&] { tail(false); });
            cg.T = T; cg.buf = A; cg.out = pcm_dev; cg.tmul = tmul;
        }
        HIP_OK(hipGraphLaunch(cg.exec.get(), s));
        c->stats.graph_replays++;
        pcm_dev = cg.out; tmul = cg.tmul;
    } else {
        tail(true);
    }
    std::vector<float> all((size_t) Ts * tmul);                  // the final conv has one output channel: utterance b = samples [tmul Tpre[b], tmul Tpre[b + 1])
    HIP_OK(hipMemcpyAsync(all.data(), pcm_dev, all.size() * 4, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    std::vector<std::vector<float>> pcm((size_t) B);
    for (int b = 0; b < B; b++) pcm[(size_t) b].assign(all.begin() + (size_t) tmul * Tpre[(size_t) b], all.begin() + (size_t) tmul * Tpre[(size_t) b + 1]);
    return pcm;
}

std::vector<float> engine_codec_decode(bark_context * c, const int32_t * codes, int n_q, int T, int tap_stage, std::vector<float> * tap) {
    return std::move(engine_codec_decode_many(c, {codes}, n_q, {T}, tap_stage, tap)[0]);
}

// EnCodec encode (HF modeling_encodec.py: EncodecEncoder, EncodecResidualVectorQuantizer.encode): PCM -> latents -> codes, for up to 32 recordings in one
// pass.  Time-major activations as in the decoder; the stages are ragged (ceil at every stride), so each stage has its own row table (d_enc_T) and every
// launch takes its stage's CodecBatch with factor 1.  The first convolution reads the f16 image of the PCM, like every other convolution operand (R1).
std::vector<std::vector<int32_t>> engine_codec_encode_many(bark_context * c, const std::vector<const float *> & pcm, const std::vector<int> & n_samples, int n_q,
                                                           int tap_stage, std::vector<float> * tap) {
    HIP_OK(hipSetDevice(c->device));
    c->enc_latents = nullptr; c->enc_latent_rows = 0;
    CodecModel & cm = c->codec;
    const CodecModel::Encoder & en = cm.enc;
    if (!en.present) throw std::runtime_error("codec: the model file holds no encoder");
    const int B = (int) n_samples.size();
    if (B < 1 || B > 32 || pcm.size() != n_samples.size()) throw std::runtime_error("codec: 1..32 recordings per call");
    if (tap_stage >= 0 && B != 1) throw std::runtime_error("codec: activation taps take one recording");
    if (tap_stage > 6) throw std::runtime_error("codec: the encoder has tap stages 0..6");
    if (n_q <= 0 || n_q > cm.n_q) throw std::runtime_error("codec: n_q outside the file's codebooks");
    // rows of every recording at the five stages, and their prefix sums: hdr[stage] = {[0, 32) rows, [40, 73) prefix sums}
    int hdr[5][80] = {};
    int ch[5]; ch[0] = en.F;
    for (int b = 0; b < B; b++) {
        const int n = n_samples[(size_t) b];
        if (n < 1 || n > 4096 * 320 || !pcm[(size_t) b]) throw std::runtime_error("codec: a recording needs 1 .. 4096 frames of samples");
        // refused at the door: a sample that is not finite, or whose f16 image - what the first convolution reads - is not (|x| >= 65520)
        for (int i = 0; i < n; i++) if (!std::isfinite(pcm[(size_t) b][i]) || !std::isfinite((float) (_Float16) pcm[(size_t) b][i])) throw std::runtime_error("codec: non-finite sample (or one beyond the f16 range)");
        int L = n;
        for (int st = 0; st < 5; st++) {
            hdr[st][b] = L; hdr[st][40 + b + 1] = hdr[st][40 + b] + L;
            if (st < 4) L = (L + en.blocks[st].stride - 1) / en.blocks[st].stride;
        }
    }
    for (int st = 0; st < 4; st++) ch[st + 1] = en.blocks[st].down.cout;
    int rows[5];
    size_t need = 0;
    for (int st = 0; st < 5; st++) { rows[st] = hdr[st][40 + B]; need = std::max(need, (size_t) rows[st] * ch[st]); }
    const int Ts = rows[4], D = cm.D, Hd = cm.hp.hidden_dim;
    int Tmax = 0;
    for (int b = 0; b < B; b++) Tmax = std::max(Tmax, hdr[4][b]);
    need = std::max(need, (size_t) Ts * std::max(D, Hd));
    hipStream_t s = c->stream;
    ensure_codec_scratch(c, need, Ts, D);
    c->d_enc_T.reserve(c, 5 * 80);
    c->d_pcm.reserve(c, (size_t) rows[0]);
    c->d_codes.reserve(c, (size_t) n_q * Ts);
    for (int b = 0; b < B; b++)
        HIP_OK(hipMemcpyAsync(c->d_pcm.p + hdr[0][40 + b], pcm[(size_t) b], (size_t) n_samples[(size_t) b] * 4, hipMemcpyHostToDevice, s));
    HIP_OK(hipMemcpyAsync(c->d_enc_T.p, hdr, sizeof(hdr), hipMemcpyHostToDevice, s));
    HIP_OK(hipStreamSynchronize(s));                            // hdr is a stack object
    CodecBatch cb[5];
    for (int st = 0; st < 5; st++) { cb[st].T = c->d_enc_T.p + 80 * st; cb[st].Tpre = c->d_enc_T.p + 80 * st + 40; cb[st].B = B; }
    float * A = c->cbuf[0].p, * Bf = c->cbuf[1].p, * R = c->cbuf[2].p;
    half_t * H0 = c->cbuf_hh[0].p, * H1 = c->cbuf_hh[1].p, * H2 = c->cbuf_hh[2].p;

    auto conv = [&](const CodecModel::Conv & cv, const half_t * xh, int st, const float * add, float * y, half_t * yh_raw, half_t * yh_elu) {
        ConvTmArgs a;
        a.W = cv.wm; a.w32 = cv.w32; a.bias = cv.b; a.cin = cv.cin; a.cout = cv.cout; a.cout32 = (cv.cout + 31) & ~31; a.K = cv.k;
        a.kd = cv.k * cv.cin; a.kd16 = (a.kd + 15) & ~15;
        a.xh = xh; a.rows_in = rows[st]; a.tm_in = 1; a.cb = cb[st];
        a.add = add; a.y = y; a.yh_raw = yh_raw; a.yh_elu = yh_elu;
        launch_conv_tm(s, a);
    };
    auto grab = [&](int stage, const float * buf, int C, size_t nrows) {
        if (tap_stage != stage || !tap) return;
        std::vector<float> tm((size_t) C * nrows);
        HIP_OK(hipMemcpyAsync(tm.data(), buf, tm.size() * 4, hipMemcpyDeviceToHost, s));
        HIP_OK(hipStreamSynchronize(s));
        tap->resize(tm.size());
        for (size_t r = 0; r < nrows; r++) for (int k = 0; k < C; k++) (*tap)[(size_t) k * nrows + r] = tm[r * (size_t) C + k];
    };
    const bool taps = tap_stage >= 0;
    c->enc_ev[0].record(s);
    launch_act_round(s, c->d_pcm.p, (size_t) rows[0], 0, H0);                  // the PCM's f16 image [rows][1]
    conv(en.init, H0, 0, nullptr, taps ? A : nullptr, H1, H2);              // H1 = f16(x): shortcut input, H2 = f16(ELU(x)): conv1 input
    grab(0, A, ch[0], (size_t) rows[0]);
    for (int b = 0; b < 4; b++) {
        const CodecModel::EncBlock & bl = en.blocks[b];
        // residual block: shortcut(x) + conv2(elu(conv1(elu(x)))), then ELU: the strided convolution's input
        conv(bl.c1, H2, b, nullptr, nullptr, nullptr, H0);
        conv(bl.c2, H0, b, nullptr, R, nullptr, nullptr);
        conv(bl.sc, H1, b, R, nullptr, nullptr, H0);
        ConvDownArgs d;
        d.W = bl.down.wm; d.w32 = bl.down.w32; d.bias = bl.down.b; d.cin = bl.down.cin; d.cout = bl.down.cout; d.cout32 = (bl.down.cout + 31) & ~31;
        d.K = bl.down.k; d.stride = bl.stride; d.kd = d.K * d.cin; d.kd16 = (d.kd + 15) & ~15;
        d.xh = H0; d.rows_out = rows[b + 1]; d.cb_in = cb[b]; d.cb_out = cb[b + 1];
        if (b < 3) { d.y = taps ? A : nullptr; d.yh_raw = H1; d.yh_elu = H2; }
        else { d.y = Bf; d.yh_raw = c->c_xt_h.p; }                            // Bf = x [row][D] for the skip; its f16 image is the LSTM's input
        launch_conv_down(s, d);
        grab(1 + b, b < 3 ? A : Bf, ch[b + 1], (size_t) rows[b + 1]);
    }
    run_lstm_pair(c, en.lstm, c->lstm_graph_enc, cb[4], Ts, Tmax, R, codec_lstm_io(c));
    launch_add(s, R, Bf, (size_t) D * Ts, A);                               // y + x
    grab(5, A, D, (size_t) Ts);
    launch_act_round(s, A, (size_t) D * Ts, 1, H0);
    conv(en.fin, H0, 4, nullptr, Bf, nullptr, nullptr);                     // Bf = latent [row][H]
    grab(6, Bf, Hd, (size_t) Ts);
    launch_rvq_encode(s, cm.codebooks, cm.hp.n_bins, Hd, Bf, n_q, Ts, c->d_codes.p, cb[4]);
    c->enc_ev[1].record(s);
    c->enc_latents = Bf; c->enc_latent_rows = Ts;
    std::vector<int32_t> all((size_t) n_q * Ts);
    HIP_OK(hipMemcpyAsync(all.data(), c->d_codes.p, all.size() * 4, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    { float ms = 0.0f; HIP_OK(hipEventElapsedTime(&ms, c->enc_ev[0].get(), c->enc_ev[1].get())); c->enc_device_us = 1e3 * ms; }
    throw_on_missing_pick(all);
    std::vector<std::vector<int32_t>> out((size_t) B);
    for (int b = 0; b < B; b++) out[(size_t) b].assign(all.begin() + (size_t) n_q * hdr[4][40 + b], all.begin() + (size_t) n_q * hdr[4][40 + b + 1]);
    return out;
}

std::vector<int32_t> engine_rvq_encode(bark_context * c, const float * latents, int T, int n_q) {
    HIP_OK(hipSetDevice(c->device));
    c->enc_latents = nullptr; c->enc_latent_rows = 0;
    CodecModel & cm = c->codec;
    if (!cm.enc.present) throw std::runtime_error("codec: the model file holds no encoder");
    if (T < 1 || T > 65536 || n_q <= 0 || n_q > cm.n_q) throw std::runtime_error("codec: bad latent shape / n_q");
    const int Hd = cm.hp.hidden_dim;
    hipStream_t s = c->stream;
    ensure_codec_scratch(c, (size_t) T * std::max(Hd, cm.D), 0, cm.D);
    c->d_enc_T.reserve(c, 5 * 80);
    c->d_codes.reserve(c, (size_t) n_q * T);
    int hdr[80] = {};
    hdr[0] = T; hdr[41] = T;
    HIP_OK(hipMemcpyAsync(c->d_enc_T.p, hdr, sizeof(hdr), hipMemcpyHostToDevice, s));
    HIP_OK(hipMemcpyAsync(c->cbuf[1].p, latents, (size_t) T * Hd * 4, hipMemcpyHostToDevice, s));
    CodecBatch cb; cb.T = c->d_enc_T.p; cb.Tpre = c->d_enc_T.p + 40; cb.B = 1;
    launch_rvq_encode(s, cm.codebooks, cm.hp.n_bins, Hd, c->cbuf[1].p, n_q, T, c->d_codes.p, cb);
    std::vector<int32_t> codes((size_t) n_q * T);
    HIP_OK(hipMemcpyAsync(codes.data(), c->d_codes.p, codes.size() * 4, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));                            // also: hdr is a stack object
    throw_on_missing_pick(codes);
    return codes;
}

}  // namespace barkhip

// ---- semantic encoder (rule C12h): 16 kHz PCM -> HuBERT hidden state -> token head -> ids ------------------------------------
namespace {
// the seven valid convolutions: kernels 10, 3, 3, 3, 3, 2, 2 with strides 5, 2, 2, 2, 2, 2, 2 - rows[0] samples, rows[i + 1] the rows behind convolution i
void hub_stage_rows(const HubertModel & hm, int n, int rows[8]) {
    rows[0] = n;
    rows[1] = (n - hm.k0) / 5 + 1;
    for (int i = 0; i < 6; i++) rows[i + 2] = (rows[i + 1] - hm.conv[i].k) / hm.conv[i].stride + 1;
}
constexpr int kHubMaxSamples = (kHubMaxFrames - 1) * 320 + 400 + 319;      // the longest input with T <= 1024: 328 079

void ensure_hub_scratch(bark_context * c) {
    bark_context::HubScratch & h = c->hubs;
    if (h.ready) return;
    const HubertModel & hm = *c->hub;
    const HubertHparams & hp = hm.hp;
    int rows[8];
    hub_stage_rows(hm, kHubMaxSamples, rows);
    const size_t T = kHubMaxFrames, C = hp.C, H = hp.H, F = hp.F, D = hp.D;
    h.pcm = dev_alloc<float>(c, kHubMaxSamples); h.pcm_h = dev_alloc<half_t>(c, kHubMaxSamples);
    h.a16 = dev_alloc<half_t>(c, (size_t) rows[1] * C); h.b16 = dev_alloc<half_t>(c, (size_t) rows[2] * C);
    h.part = dev_alloc<double>(c, (size_t) hub_conv0_chunks(rows[1]) * C * 2); h.stats = dev_alloc<float>(c, 2 * C);
    h.feat = dev_alloc<float>(c, T * C);
    h.x = dev_alloc<float>(c, T * H); h.tmp = dev_alloc<float>(c, T * H); h.q = dev_alloc<float>(c, T * H);
    h.kc = dev_alloc<float>(c, T * H); h.vc = dev_alloc<float>(c, T * H);
    h.xh = dev_alloc<half_t>(c, T * std::max(C, H)); h.att = dev_alloc<half_t>(c, T * H); h.hb = dev_alloc<half_t>(c, T * F);
    h.gi = dev_alloc<float>(c, T * 4 * D); h.c1 = dev_alloc<float>(c, D); h.c2 = dev_alloc<float>(c, D); h.out2 = dev_alloc<float>(c, T * D);
    h.h1 = dev_alloc<half_t>(c, T * D); h.h2 = dev_alloc<half_t>(c, T * D);
    h.logits = dev_alloc<float>(c, T * hp.n_classes); h.ids = dev_alloc<int32_t>(c, T);
    h.rows = dev_alloc<int>(c, 8 * 80);
    h.ready = true;
}

// token head on the f16 rows h.xh [T][H]: two LSTM layers (the codec's wave front), linear layer, per-row pick -> h.logits, h.ids
void run_token_head(bark_context * c, int T) {
    const HubertModel & hm = *c->hub;
    bark_context::HubScratch & h = c->hubs;
    hipStream_t s = c->stream;
    const int D = hm.hp.D, NC = hm.hp.n_classes;
    CodecBatch one;                                              // one recording: the launch's own T
    run_lstm_pair(c, hm.lstm, c->lstm_graph_hub, one, T, T, h.out2, LstmIo{h.xh, hm.hp.H, D, h.gi, h.c1, h.c2, h.h1, h.h2});
    LinArgs o;
    o.W = hm.out_w; o.M = NC; o.K = D; o.N = T; o.x_f16 = h.h2; o.bias = hm.out_b; o.epi = EPI_LOGITS; o.out = h.logits; o.ld_out = NC;
    launch_linear(s, o);
    launch_argmax_rows(s, h.logits, NC, T, NC, h.ids, 1, nullptr);
}
}  // namespace

namespace barkhip {

std::vector<int32_t> engine_semantic_head(bark_context * c, const float * feats, int T, std::vector<float> * logits) {
    HIP_OK(hipSetDevice(c->device));
    if (!c->hub) throw std::runtime_error("semantic encoder: none loaded");
    if (!feats || T < 1 || T > kHubMaxFrames) throw std::runtime_error("semantic encoder: the head takes 1 .. 1024 frames");
    const HubertHparams & hp = c->hub->hp;
    for (size_t i = 0; i < (size_t) T * hp.H; i++) if (!std::isfinite((float) (_Float16) feats[i])) throw std::runtime_error("semantic encoder: non-finite feature (or one beyond the f16 range)");
    ensure_hub_scratch(c);
    bark_context::HubScratch & h = c->hubs;
    hipStream_t s = c->stream;
    HIP_OK(hipMemcpyAsync(h.x, feats, (size_t) T * hp.H * 4, hipMemcpyHostToDevice, s));
    launch_act_round(s, h.x, (size_t) T * hp.H, 0, h.xh);
    run_token_head(c, T);
    std::vector<int32_t> ids((size_t) T);
    if (logits) { logits->resize((size_t) T * hp.n_classes); HIP_OK(hipMemcpyAsync(logits->data(), h.logits, logits->size() * 4, hipMemcpyDeviceToHost, s)); }
    HIP_OK(hipMemcpyAsync(ids.data(), h.ids, ids.size() * 4, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    return ids;
}

std::vector<int32_t> engine_semantic_encode(bark_context * c, const float * pcm, int n, int tap_stage, std::vector<float> * tap) {
    HIP_OK(hipSetDevice(c->device));
    if (!c->hub) throw std::runtime_error("semantic encoder: none loaded");
    const HubertModel & hm = *c->hub;
    const HubertHparams & hp = hm.hp;
    if (tap_stage > 5) throw std::runtime_error("semantic encoder: tap stages are 0..5");
    if (!pcm || n < 400) throw std::runtime_error("semantic encoder: a recording needs at least 400 samples (one frame)");
    if (n > kHubMaxSamples) throw std::runtime_error("semantic encoder: more than 1024 frames (328 079 samples) are refused");
    for (int i = 0; i < n; i++) if (!std::isfinite(pcm[i]) || !std::isfinite((float) (_Float16) pcm[i])) throw std::runtime_error("semantic encoder: non-finite sample (or one beyond the f16 range)");
    int rows[8];
    hub_stage_rows(hm, n, rows);
    const int T = rows[7], T0 = rows[1], C = hp.C, H = hp.H, F = hp.F;
    if (T != (n - 400) / 320 + 1 || T < 1 || T > kHubMaxFrames) throw std::runtime_error("semantic encoder: frame count outside 1 .. 1024");
    ensure_hub_scratch(c);
    bark_context::HubScratch & h = c->hubs;
    hipStream_t s = c->stream;
    const bool taps = tap_stage >= 0;
    if (tap_stage == 0) h.tap.reserve(c, (size_t) T0 * C);
    {
        int hdr[8][80] = {};
        for (int st = 0; st < 8; st++) { hdr[st][0] = rows[st]; hdr[st][41] = rows[st]; }
        HIP_OK(hipMemcpyAsync(h.rows, hdr, sizeof(hdr), hipMemcpyHostToDevice, s));
        HIP_OK(hipMemcpyAsync(h.pcm, pcm, (size_t) n * 4, hipMemcpyHostToDevice, s));
        HIP_OK(hipStreamSynchronize(s));                        // hdr is a stack object
    }
    auto stage_cb = [&](int st) { CodecBatch cb; cb.T = h.rows + 80 * st; cb.Tpre = h.rows + 80 * st + 40; cb.B = 1; return cb; };
    auto grab = [&](int stage, const float * buf, size_t elems) {
        if (tap_stage != stage || !tap) return;
        tap->resize(elems);
        HIP_OK(hipMemcpyAsync(tap->data(), buf, elems * 4, hipMemcpyDeviceToHost, s));
        HIP_OK(hipStreamSynchronize(s));
    };
    c->hub_ev[0].record(s);
    // feature encoder: the f16 image of the samples, convolution 0 + norm + GELU, six valid convolutions on the matrix cores (a16 <-> b16)
    launch_act_round(s, h.pcm, (size_t) n, 0, h.pcm_h);
    {
        HubConv0Args a;
        a.xh = h.pcm_h; a.n = n; a.T0 = T0; a.w = hm.conv0_w; a.C = C; a.K = hm.k0; a.stride = 5;
        a.part = h.part; a.stats = h.stats; a.g = hm.gn_g; a.b = hm.gn_b; a.yh = h.a16; a.y = tap_stage == 0 ? h.tap.p : nullptr;
        launch_hub_conv0(s, a);
    }
    grab(0, h.tap.p, (size_t) T0 * C);
    half_t * src = h.a16, * dst = h.b16;
    for (int i = 0; i < 6; i++) {
        const HubertModel::Conv & cv = hm.conv[i];
        ConvDownArgs d;
        d.W = cv.wm; d.w32 = cv.w32; d.bias = nullptr; d.cin = C; d.cout = C; d.cout32 = (C + 31) & ~31;
        d.K = cv.k; d.stride = cv.stride; d.kd = cv.k * C; d.kd16 = (d.kd + 15) & ~15; d.valid = 1;
        d.xh = src; d.rows_out = rows[i + 2]; d.cb_in = stage_cb(i + 1); d.cb_out = stage_cb(i + 2);
        if (i < 5) d.yh_gelu = dst; else d.y_gelu = h.feat;     // the last one feeds a LayerNorm: f32
        launch_conv_down(s, d);
        std::swap(src, dst);
    }
    grab(1, h.feat, (size_t) T * C);
    // projection: LayerNorm(C) -> f16 rows -> Linear(C -> H)
    launch_add_ln_rows(s, h.feat, nullptr, T, C, hm.fp_ln_g, hm.fp_ln_b, nullptr, h.xh);
    {
        LinArgs p;
        p.W = hm.fp_w; p.M = H; p.K = C; p.N = T; p.x_f16 = h.xh; p.bias = hm.fp_b; p.epi = EPI_LOGITS; p.out = h.x; p.ld_out = H;
        launch_linear(s, p);
    }
    grab(2, h.x, (size_t) T * H);
    // positional convolution on the f16 image of the projection, GELU, + projection, encoder.layer_norm -> hidden_states[0]
    launch_act_round(s, h.x, (size_t) T * H, 0, h.xh);
    {
        PosConvArgs p;
        p.W = hm.pos_w; p.bias = hm.pos_b; p.xh = h.xh; p.T = T; p.H = H; p.G = hp.pos_groups; p.Kp = hp.pos_kernel;
        p.kd = hm.pos_kd; p.kd16 = hm.pos_kd16; p.co32 = hm.pos_co32; p.y = h.tmp;
        launch_pos_conv(s, p);
    }
    launch_add_ln_rows(s, h.x, h.tmp, T, H, hm.enc_ln_g, hm.enc_ln_b, h.x, h.xh);
    grab(3, h.x, (size_t) T * H);
    // layers 1 .. L (post-norm): attention over all T frames, residual, LayerNorm; FFN with erf GELU, residual, LayerNorm
    for (const HubertModel::Layer & ly : hm.layers) {
        LinArgs qkv;
        qkv.W = ly.qkv_w; qkv.M = 3 * H; qkv.K = H; qkv.N = T; qkv.x_f16 = h.xh; qkv.bias = ly.qkv_b; qkv.epi = EPI_QKV;
        qkv.q = h.q; qkv.kc = h.kc; qkv.vc = h.vc; qkv.E = H; qkv.P = kHubMaxFrames; qkv.pos0 = 0;
        launch_linear(s, qkv);
        AttnPrefillArgs at;
        at.q = h.q; at.ldq = H; at.kc = h.kc; at.vc = h.vc; at.H = hp.n_head; at.P = kHubMaxFrames; at.N = T; at.n_past = 0; at.causal = 0;
        at.att = h.att; at.ld_att = H;
        launch_attn_prefill(s, at);
        LinArgs o;
        o.W = ly.o_w; o.M = H; o.K = H; o.N = T; o.x_f16 = h.att; o.bias = ly.o_b; o.epi = EPI_LOGITS; o.out = h.tmp; o.ld_out = H;
        launch_linear(s, o);
        launch_add_ln_rows(s, h.x, h.tmp, T, H, ly.ln1_g, ly.ln1_b, h.x, h.xh);
        LinArgs f1;
        f1.W = ly.fc1_w; f1.M = F; f1.K = H; f1.N = T; f1.x_f16 = h.xh; f1.bias = ly.fc1_b; f1.epi = EPI_GELU; f1.out_h = h.hb; f1.lut = hm.gelu_erf_lut;
        launch_linear(s, f1);
        LinArgs f2;
        f2.W = ly.fc2_w; f2.M = H; f2.K = F; f2.N = T; f2.x_f16 = h.hb; f2.bias = ly.fc2_b; f2.epi = EPI_LOGITS; f2.out = h.tmp; f2.ld_out = H;
        launch_linear(s, f2);
        launch_add_ln_rows(s, h.x, h.tmp, T, H, ly.ln2_g, ly.ln2_b, h.x, h.xh);
    }
    grab(4, h.x, (size_t) T * H);
    run_token_head(c, T);
    c->hub_ev[1].record(s);
    grab(5, h.logits, (size_t) T * hp.n_classes);
    std::vector<int32_t> ids((size_t) T);
    HIP_OK(hipMemcpyAsync(ids.data(), h.ids, ids.size() * 4, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    if (!taps) { float ms = 0.0f; HIP_OK(hipEventElapsedTime(&ms, c->hub_ev[0].get(), c->hub_ev[1].get())); c->hub_device_us = 1e3 * ms; }
    return ids;
}

// ---- voice prompts from a recording: the resampler (rule C13r) and the composition of the three streams ----------------------------------------------
std::vector<float> engine_resample_24k_16k(bark_context * c, const float * pcm, int n) {
    HIP_OK(hipSetDevice(c->device));
    if (!pcm || n < 1 || n > kResampleMaxSamples) throw std::runtime_error("resampler: a recording needs 1 .. 1 310 720 samples (4096 codec frames)");
    for (int i = 0; i < n; i++) if (!std::isfinite(pcm[i])) throw std::runtime_error("resampler: non-finite sample");
    const int n_out = (2 * n + 2) / 3;
    c->rs_in.reserve(c, (size_t) n); c->rs_out.reserve(c, (size_t) n_out);
    hipStream_t s = c->stream;
    HIP_OK(hipMemcpyAsync(c->rs_in.p, pcm, (size_t) n * 4, hipMemcpyHostToDevice, s));
    launch_resample_24k_16k(s, c->rs_in.p, n, c->rs_out.p, n_out);
    std::vector<float> out((size_t) n_out);
    HIP_OK(hipMemcpyAsync(out.data(), c->rs_out.p, out.size() * 4, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    return out;
}

double engine_time_resample(bark_context * c, int n, int iters) {
    HIP_OK(hipSetDevice(c->device));
    if (n < 1 || n > kResampleMaxSamples) throw std::runtime_error("time_resample: 1 .. 1 310 720 samples");
    const int n_out = (2 * n + 2) / 3;
    c->rs_in.reserve(c, (size_t) n); c->rs_out.reserve(c, (size_t) n_out);
    HIP_OK(hipMemsetAsync(c->rs_in.p, 0, (size_t) n * 4, c->stream));      // the time does not depend on the values
    iters = std::max(1, iters);
    for (int i = 0; i < 2; i++) launch_resample_24k_16k(c->stream, c->rs_in.p, n, c->rs_out.p, n_out);
    return time_on_stream_us(c, [&] { for (int i = 0; i < iters; i++) launch_resample_24k_16k(c->stream, c->rs_in.p, n, c->rs_out.p, n_out); }) / iters;
}

// ---- output rate and sample format: the rational resampler (rule C14r) ------------------------------------------------------------------------------------
namespace {
constexpr int kPairRates[8] = {8000, 12000, 16000, 22050, 24000, 32000, 44100, 48000};
bool pair_rate(int r) { for (int v : kPairRates) if (v == r) return true; return false; }
int gcd_int(int a, int b) { while (b) { const int t = a % b; a = b; b = t; } return a; }
// numpy's sinc: sin(pi x) / (pi x) with x = 0 moved to 1e-20 (the quotient is then exactly 1)
double np_sinc(double x) { const double y = M_PI * (x == 0.0 ? 1.0e-20 : x); return sin(y) / y; }
ResampleTable make_pair_table(int rate_in, int rate_out) {
    ResampleTable t;
    const int g = gcd_int(rate_in, rate_out);
    t.L = rate_out / g; t.M = rate_in / g;
    const double c = 0.99 * std::min(1.0, (double) t.L / (double) t.M), W = 6.0 / c;
    t.half = (int) ceil(W) + 1;
    const int nt = 2 * t.half;
    t.h.resize((size_t) t.L * nt);
    if (rate_in == 24000 && rate_out == 16000) {                // C13r's committed table IS this pair's table
        if (t.L != 2 || nt != 22) throw std::runtime_error("resampler: the committed 24000 -> 16000 table does not have the rule's shape");
        std::copy(resample_taps(), resample_taps() + 44, t.h.begin());
        return t;
    }
    // every step in double, in the expression order of voice.resample_24k_to_16k / tests/resample_ref.py (this file is compiled without contraction)
    for (int p = 0; p < t.L; p++) for (int k = 0; k < nt; k++) {
        const double u = (double) p / (double) t.L - (double) (k - t.half + 1);
        const double s = c * np_sinc(c * u);
        double win = 0.0;
        if (fabs(u) < W) { const double co = cos(M_PI * u / (2.0 * W)); win = co * co; }
        t.h[(size_t) p * nt + k] = (float) (s * win);
    }
    return t;
}
}  // namespace

bool resample_pair_supported(int rate_in, int rate_out) { return pair_rate(rate_in) && pair_rate(rate_out) && (rate_in == 24000 || rate_out == 24000); }

const ResampleTable * resample_pair_table(int rate_in, int rate_out) {
    if (!resample_pair_supported(rate_in, rate_out) || rate_in == rate_out) return nullptr;
    static std::mutex mu;
    static std::map<std::pair<int, int>, ResampleTable> cache;          // entries are never removed: the pointers stay valid
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache.find({rate_in, rate_out});
    if (it == cache.end()) it = cache.emplace(std::make_pair(rate_in, rate_out), make_pair_table(rate_in, rate_out)).first;
    return &it->second;
}

long long resample_out_len(long long n, int rate_in, int rate_out) {
    if (n < 0 || !resample_pair_supported(rate_in, rate_out)) return -1;
    if (rate_in == rate_out) return n;
    const int g = gcd_int(rate_in, rate_out);
    const long long L = rate_out / g, M = rate_in / g;
    return (n * L + M - 1) / M;
}

namespace {
// the device copy of a pair's taps, uploaded with the context's first use of the pair
const float * device_taps(bark_context * c, int rate_in, int rate_out, const ResampleTable & t) {
    auto it = c->rp_taps.find({rate_in, rate_out});
    if (it != c->rp_taps.end()) return it->second;
    float * d = dev_alloc<float>(c, t.h.size());
    HIP_OK(hipMemcpyAsync(d, t.h.data(), t.h.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    c->rp_taps[{rate_in, rate_out}] = d;
    return d;
}
// FLAC (rule C18f): the device half of the encoder, defined with engine_flac_encode_many below
std::vector<uint8_t> flac_staged(bark_context * c, const int16_t * dx, const int * n, int count, int rate, std::vector<int32_t> & lengths, std::vector<int32_t> * frames);
void ensure_resample_buffers(bark_context * c, size_t in_elems, size_t out_bytes) {
    c->rp_in.reserve(c, in_elems);
    c->rp_out.reserve(c, out_bytes);
    c->rp_seg.reserve(c, 5 * (kResampleMaxSegments + 1));
}
// the segment table of launch_resample_pair for `count` segments of n[i] samples; returns the tile count
int fill_segment_table(int (&seg)[5][kResampleMaxSegments + 1], const int * n, int count, int rate_in, int rate_out, std::vector<int32_t> & n_out) {
    memset(seg, 0, sizeof(seg));
    n_out.assign((size_t) count, 0);
    for (int i = 0; i < count; i++) {
        n_out[(size_t) i] = (int32_t) resample_out_len(n[i], rate_in, rate_out);
        seg[0][i] = n[i]; seg[2][i] = n_out[(size_t) i];
        seg[1][i + 1] = seg[1][i] + n[i]; seg[3][i + 1] = seg[3][i] + n_out[(size_t) i];
        seg[4][i + 1] = seg[4][i] + (n_out[(size_t) i] + kResampleTile - 1) / kResampleTile;
    }
    return seg[4][count];
}
// the device half of a conversion: `count` segments lie back to back at dx (total_in samples) -> out (sized by the caller) in fmt; t == nullptr: no filter
void convert_staged(bark_context * c, const float * dx, const int (&seg)[5][kResampleMaxSegments + 1], int n_tiles, int count, size_t total_in,
                    const ResampleTable * t, int rate_in, int rate_out, int fmt, std::vector<uint8_t> & out) {
    hipStream_t s = c->stream;
    if (!t) launch_sample_format(s, dx, c->rp_out.p, total_in, pcm_format(fmt));
    else {
        HIP_OK(hipMemcpyAsync(c->rp_seg.p, seg, sizeof(seg), hipMemcpyHostToDevice, s));
        ResamplePairArgs a;
        a.x = dx; a.y = c->rp_out.p; a.taps = device_taps(c, rate_in, rate_out, *t); a.seg = c->rp_seg.p;
        a.B = count; a.L = t->L; a.M = t->M; a.half = t->half; a.fmt = pcm_format(fmt);
        launch_resample_pair(s, a, n_tiles);
    }
    if (fmt == BARK_HIP_SAMPLE_FLAC) {                           // the s16 samples stay where they are: only the streams return (the call synchronises)
        out = flac_staged(c, reinterpret_cast<const int16_t *>(c->rp_out.p), seg[2], count, rate_out, c->flac_lengths, nullptr);
        return;
    }
    HIP_OK(hipMemcpyAsync(out.data(), c->rp_out.p, out.size(), hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));                             // seg is a stack object of the caller
}
}  // namespace

std::vector<uint8_t> engine_resample_many(bark_context * c, const float * const * pcm, const int * n, int count, int rate_in, int rate_out, int fmt,
                                          std::vector<int32_t> & n_out) {
    HIP_OK(hipSetDevice(c->device));
    if (!pcm || !n || count < 1 || count > kResampleMaxSegments) throw std::runtime_error("resampler: 1 .. 64 segments in one call");
    if (!resample_pair_supported(rate_in, rate_out)) throw std::runtime_error("resampler: the rates are 8000, 12000, 16000, 22050, 24000, 32000, 44100 and 48000, with 24000 on at least one side");
    const int bytes_per = render_format_bytes(fmt);
    if (!bytes_per) throw std::runtime_error("resampler: the sample formats are f32 (0), s16 (1), mu-law (2) and FLAC (3)");
    size_t total_in = 0;
    for (int i = 0; i < count; i++) {
        if (!pcm[i] || n[i] < 1 || n[i] > kResampleMaxSamples) throw std::runtime_error("resampler: a segment needs 1 .. 1 310 720 samples");
        for (int k = 0; k < n[i]; k++) if (!std::isfinite(pcm[i][k])) throw std::runtime_error("resampler: non-finite sample");
        total_in += (size_t) n[i];
    }
    int seg[5][kResampleMaxSegments + 1];
    const int n_tiles = fill_segment_table(seg, n, count, rate_in, rate_out, n_out);
    const size_t total_out = (size_t) seg[3][count];
    std::vector<uint8_t> out(total_out * (size_t) bytes_per);
    const ResampleTable * t = resample_pair_table(rate_in, rate_out);
    if (!t && fmt == BARK_HIP_SAMPLE_F32) {                      // the identity in f32: no filter, no launch, the samples themselves
        for (int i = 0; i < count; i++) memcpy(out.data() + (size_t) seg[3][i] * 4, pcm[i], (size_t) n[i] * 4);
        return out;
    }
    ensure_resample_buffers(c, total_in, out.size());
    hipStream_t s = c->stream;
    for (int i = 0; i < count; i++) HIP_OK(hipMemcpyAsync(c->rp_in.p + seg[1][i], pcm[i], (size_t) n[i] * 4, hipMemcpyHostToDevice, s));
    convert_staged(c, c->rp_in.p, seg, n_tiles, count, total_in, t, rate_in, rate_out, fmt, out);
    return out;
}

double engine_time_resample_pair(bark_context * c, int n, int rate_in, int rate_out, int fmt, int iters) {
    HIP_OK(hipSetDevice(c->device));
    if (n < 1 || n > kResampleMaxSamples) throw std::runtime_error("time_resample_pair: 1 .. 1 310 720 samples");
    const ResampleTable * t = resample_pair_table(rate_in, rate_out);
    const int bytes_per = sample_format_bytes(fmt);
    if (!t || !bytes_per) throw std::runtime_error("time_resample_pair: one of the 14 pairs with a filter and a sample format 0 .. 2");
    int seg[5][kResampleMaxSegments + 1];
    std::vector<int32_t> n_out;
    const int n_tiles = fill_segment_table(seg, &n, 1, rate_in, rate_out, n_out);
    ensure_resample_buffers(c, (size_t) n, (size_t) n_out[0] * (size_t) bytes_per);
    HIP_OK(hipMemsetAsync(c->rp_in.p, 0, (size_t) n * 4, c->stream));      // the time does not depend on the values
    HIP_OK(hipMemcpyAsync(c->rp_seg.p, seg, sizeof(seg), hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    ResamplePairArgs a;
    a.x = c->rp_in.p; a.y = c->rp_out.p; a.taps = device_taps(c, rate_in, rate_out, *t); a.seg = c->rp_seg.p;
    a.B = 1; a.L = t->L; a.M = t->M; a.half = t->half; a.fmt = fmt;
    iters = std::max(1, iters);
    for (int i = 0; i < 2; i++) launch_resample_pair(c->stream, a, n_tiles);
    return time_on_stream_us(c, [&] { for (int i = 0; i < iters; i++) launch_resample_pair(c->stream, a, n_tiles); }) / iters;
}

// ---- long-form join (rule C15j) -----------------------------------------------------------------------------------------------------------------------------
namespace {
constexpr int kJoinSegInts = 3 * (kResampleMaxSegments + 1), kJoinActAt = 196, kJoinPosAt = kJoinActAt + 2 * kResampleMaxSegments,
              kJoinTabInts = kJoinPosAt + 3 * kResampleMaxSegments;
static_assert(kJoinActAt >= kJoinSegInts, "the activity table starts behind the segment table");
// the segment table of launch_segment_activity; returns the frame count
int fill_activity_table(int (&seg)[3][kResampleMaxSegments + 1], const int * n, int count) {
    memset(seg, 0, sizeof(seg));
    for (int i = 0; i < count; i++) {
        seg[0][i] = n[i];
        seg[1][i + 1] = seg[1][i] + n[i];
        seg[2][i + 1] = seg[2][i] + (n[i] + kJoinFrame - 1) / kJoinFrame;
    }
    return seg[2][count];
}
// what the join kernel reads and the caller is told: from the segments' active frames (act: -first, last; last < 0: none) to the ranges of J
struct JoinPlan { int pos[3][kResampleMaxSegments]; int R = 0; long long N = 0; std::vector<int32_t> layout; };
JoinPlan plan_join(const int * n, const int * in_off, const int * act, int count, const bark_hip_join_params & p) {
    JoinPlan pl;
    memset(pl.pos, 0, sizeof(pl.pos));
    pl.layout.assign((size_t) count * 2, 0);
    for (int i = 0; i < count; i++) {
        long long a = 0, b = 0;
        if (act[2 * i + 1] >= 0) {
            const long long fa = -(long long) act[2 * i], fb = act[2 * i + 1];
            a = kJoinFrame * std::max(fa - p.trim_pad_frames, 0LL);
            b = std::min(kJoinFrame * (fb + 1 + p.trim_pad_frames), (long long) n[i]);
        }
        if (b > a) {
            if (pl.R) pl.N += p.gap_samples;
            if (pl.N + (b - a) > kJoinMaxSamples) throw std::runtime_error("join: the joined signal would pass 2^25 samples");
            pl.pos[0][pl.R] = (int) pl.N; pl.pos[1][pl.R] = (int) (b - a); pl.pos[2][pl.R] = in_off[i] + (int) a;
            pl.R++;
        }
        pl.layout[(size_t) i * 2] = (int32_t) pl.N; pl.layout[(size_t) i * 2 + 1] = (int32_t) (b - a);
        pl.N += b - a;
    }
    return pl;
}
// the device copy of the fade table W[k] = (float) (0.5 - 0.5 cos(pi (k + 0.5) / F)): formed in double, rounded once, kept until another F is asked for
const float * device_fade(bark_context * c, int F) {
    if (F < 1) return nullptr;
    if (c->jn_fade_F != F) {
        std::vector<float> w((size_t) F);
        for (int k = 0; k < F; k++) w[(size_t) k] = (float) (0.5 - 0.5 * cos(M_PI * ((double) k + 0.5) / (double) F));
        c->jn_fade_F = -1;
        c->jn_fade.reserve(c, (size_t) kJoinMaxFade);
        HIP_OK(hipMemcpyAsync(c->jn_fade.p, w.data(), w.size() * 4, hipMemcpyHostToDevice, c->stream));
        HIP_OK(hipStreamSynchronize(c->stream));                 // w is a local
        c->jn_fade_F = F;
    }
    return c->jn_fade.p;
}
// the join kernel's arguments for a plan; L = M = half = 1 without a table (the identity)
JoinResampleArgs join_args(bark_context * c, const JoinPlan & pl, const bark_hip_join_params & p, int rate_out, int fmt) {
    JoinResampleArgs a;
    const ResampleTable * t = resample_pair_table(24000, rate_out);
    a.x = c->rp_in.p; a.y = c->rp_out.p; a.pos = c->jn_tab.p + kJoinPosAt; a.fade = device_fade(c, p.fade_samples);
    a.taps = t ? device_taps(c, 24000, rate_out, *t) : nullptr;
    a.R = pl.R; a.F = p.fade_samples; a.N = (int) pl.N; a.n_out = (int) resample_out_len(pl.N, 24000, rate_out); a.fmt = pcm_format(fmt);
    if (t) { a.L = t->L; a.M = t->M; a.half = t->half; }
    return a;
}
}  // namespace

bool join_params_valid(const bark_hip_join_params & p) {
    return p.gap_samples >= 0 && p.fade_samples >= 0 && p.fade_samples <= kJoinMaxFade && std::isfinite(p.trim_threshold) && p.trim_threshold >= 0.0f && p.trim_pad_frames >= 0;
}

namespace {
// the join, or (layout_only) its first half: the checks, the active frames and the layout of J, without staging or filtering a sample
std::vector<uint8_t> join_impl(bark_context * c, const float * const * pcm, const int * n, int count, const bark_hip_join_params & p, int rate_out, int fmt,
                               std::vector<int32_t> & layout, bool layout_only) {
    HIP_OK(hipSetDevice(c->device));
    if (!pcm || !n || count < 1 || count > kResampleMaxSegments) throw std::runtime_error("join: 1 .. 64 segments in one call");
    if (!join_params_valid(p)) throw std::runtime_error("join: gap_samples >= 0, fade_samples 0 .. 24000, trim_threshold >= 0 and finite, trim_pad_frames >= 0");
    if (!resample_pair_supported(24000, rate_out)) throw std::runtime_error("join: the rates are 8000, 12000, 16000, 22050, 24000, 32000, 44100 and 48000");
    const int bytes_per = render_format_bytes(fmt);
    if (!bytes_per) throw std::runtime_error("join: the sample formats are f32 (0), s16 (1), mu-law (2) and FLAC (3)");
    long long total_in = 0;
    for (int i = 0; i < count; i++) {
        if (!pcm[i] || n[i] < 1 || n[i] > kResampleMaxSamples) throw std::runtime_error("join: a segment needs 1 .. 1 310 720 samples");
        total_in += n[i];
    }
    if (p.trim_threshold == 0.0f && total_in + (long long) (count - 1) * p.gap_samples > kJoinMaxSamples)      // nothing is trimmed: known before any work
        throw std::runtime_error("join: the joined signal would pass 2^25 samples");
    for (int i = 0; i < count; i++) for (int k = 0; k < n[i]; k++) if (!std::isfinite(pcm[i][k])) throw std::runtime_error("join: non-finite sample");
    int seg[3][kResampleMaxSegments + 1], act[2 * kResampleMaxSegments];
    const int n_frames = fill_activity_table(seg, n, count);
    const bool trim = p.trim_threshold > 0.0f;                  // threshold 0: every frame is active, the host knows the table - no activity launch, no read-back
    hipStream_t s = c->stream;
    if (trim || !layout_only) {
        c->rp_in.reserve(c, (size_t) total_in);
        c->jn_tab.reserve(c, (size_t) kJoinTabInts);
        for (int i = 0; i < count; i++) HIP_OK(hipMemcpyAsync(c->rp_in.p + seg[1][i], pcm[i], (size_t) n[i] * 4, hipMemcpyHostToDevice, s));
    }
    if (trim) {
        HIP_OK(hipMemcpyAsync(c->jn_tab.p, seg, sizeof(seg), hipMemcpyHostToDevice, s));
        HIP_OK(hipMemsetAsync(c->jn_tab.p + kJoinActAt, kJoinActFill, sizeof(act), s));
        JoinActivityArgs aa;
        aa.x = c->rp_in.p; aa.seg = c->jn_tab.p; aa.act = c->jn_tab.p + kJoinActAt; aa.B = count; aa.thr = p.trim_threshold;
        launch_segment_activity(s, aa, n_frames);
        HIP_OK(hipMemcpyAsync(act, c->jn_tab.p + kJoinActAt, (size_t) count * 8, hipMemcpyDeviceToHost, s));
        HIP_OK(hipStreamSynchronize(s));
    } else {
        for (int i = 0; i < count; i++) { act[2 * i] = 0; act[2 * i + 1] = seg[2][i + 1] - seg[2][i] - 1; }
    }
    const JoinPlan pl = plan_join(n, seg[1], act, count, p);
    layout = pl.layout;
    if (pl.N == 0 || layout_only) return {};                     // (N == 0 needs a threshold: the uploads are behind the read-back's synchronisation)
    const long long n_out = resample_out_len(pl.N, 24000, rate_out);
    std::vector<uint8_t> out((size_t) n_out * (size_t) bytes_per);
    c->rp_out.reserve(c, out.size());
    HIP_OK(hipMemcpyAsync(c->jn_tab.p + kJoinPosAt, pl.pos, sizeof(pl.pos), hipMemcpyHostToDevice, s));
    launch_join_resample(s, join_args(c, pl, p, rate_out, fmt));
    if (fmt == BARK_HIP_SAMPLE_FLAC) {                           // one stream over the joined signal
        const int n_joined = (int) n_out;
        return flac_staged(c, reinterpret_cast<const int16_t *>(c->rp_out.p), &n_joined, 1, rate_out, c->flac_lengths, nullptr);
    }
    HIP_OK(hipMemcpyAsync(out.data(), c->rp_out.p, out.size(), hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    return out;
}
}  // namespace

std::vector<uint8_t> engine_join_many(bark_context * c, const float * const * pcm, const int * n, int count, const bark_hip_join_params & p, int rate_out, int fmt,
                                      std::vector<int32_t> & layout) {
    return join_impl(c, pcm, n, count, p, rate_out, fmt, layout, false);
}

std::vector<int32_t> engine_join_layout(bark_context * c, const float * const * pcm, const int * n, int count, const bark_hip_join_params & p) {
    std::vector<int32_t> layout;
    join_impl(c, pcm, n, count, p, 24000, BARK_HIP_SAMPLE_F32, layout, true);
    return layout;
}

double engine_time_join(bark_context * c, int count, int n_each, int rate_out, int fmt, int iters, bool activity) {
    HIP_OK(hipSetDevice(c->device));
    const bark_hip_join_params p = join_default_params();
    const int bytes_per = sample_format_bytes(fmt);
    if (count < 1 || count > kResampleMaxSegments || n_each < 1 || n_each > kResampleMaxSamples || !resample_pair_supported(24000, rate_out) || !bytes_per ||
        (long long) count * n_each + (long long) (count - 1) * p.gap_samples > kJoinMaxSamples)
        throw std::runtime_error("time_join: 1 .. 64 segments of 1 .. 1 310 720 samples, 2^25 joined samples at most, a supported rate and format");
    std::vector<int> n((size_t) count, n_each), act((size_t) count * 2);
    int seg[3][kResampleMaxSegments + 1];
    const int n_frames = fill_activity_table(seg, n.data(), count);
    for (int i = 0; i < count; i++) { act[(size_t) i * 2] = 0; act[(size_t) i * 2 + 1] = seg[2][i + 1] - seg[2][i] - 1; }      // every frame is active at threshold 0
    const JoinPlan pl = plan_join(n.data(), seg[1], act.data(), count, p);
    c->rp_in.reserve(c, (size_t) count * (size_t) n_each);
    c->rp_out.reserve(c, (size_t) resample_out_len(pl.N, 24000, rate_out) * (size_t) bytes_per);
    c->jn_tab.reserve(c, (size_t) kJoinTabInts);
    hipStream_t s = c->stream;
    HIP_OK(hipMemsetAsync(c->rp_in.p, 0, (size_t) count * (size_t) n_each * 4, s));      // the time does not depend on the values
    HIP_OK(hipMemcpyAsync(c->jn_tab.p, seg, sizeof(seg), hipMemcpyHostToDevice, s));
    HIP_OK(hipMemcpyAsync(c->jn_tab.p + kJoinPosAt, pl.pos, sizeof(pl.pos), hipMemcpyHostToDevice, s));
    HIP_OK(hipStreamSynchronize(s));
    JoinActivityArgs aa;
    aa.x = c->rp_in.p; aa.seg = c->jn_tab.p; aa.act = c->jn_tab.p + kJoinActAt; aa.B = count; aa.thr = 0.0f;
    const JoinResampleArgs ja = join_args(c, pl, p, rate_out, fmt);
    // the join launch - all the device work of a call with the default parameters (threshold 0 runs no activity launch) - or, apart from it, what a
    // threshold adds in front: the activity table's fill and the activity launch, with every frame active (each one reaches for its segment's entries)
    auto one = [&] {
        if (!activity) { launch_join_resample(s, ja); return; }
        HIP_OK(hipMemsetAsync(c->jn_tab.p + kJoinActAt, kJoinActFill, (size_t) count * 8, s));
        launch_segment_activity(s, aa, n_frames);
    };
    iters = std::max(1, iters);
    for (int i = 0; i < 2; i++) one();
    return time_on_stream_us(c, [&] { for (int i = 0; i < iters; i++) one(); }) / iters;
}

// ---- speaking rate (rule C16t) ---------------------------------------------------------------------------------------------------------------------------
long long tempo_out_len(long long n, int p) {
    if (n < 1 || n > kResampleMaxSamples || p < kTempoMinSpeed || p > kTempoMaxSpeed) return -1;
    return (1000 * n + p - 1) / p;
}
namespace {
// the segment table of launch_tempo; returns the total frame count
int fill_tempo_table(int (&seg)[6][kResampleMaxSegments + 1], const int * n, const int32_t * speed, int count) {
    memset(seg, 0, sizeof(seg));
    for (int i = 0; i < count; i++) {
        const int n_out = (int) tempo_out_len(n[i], speed[i]);
        seg[0][i] = n[i]; seg[2][i] = n_out; seg[4][i] = speed[i];
        seg[1][i + 1] = seg[1][i] + n[i]; seg[3][i + 1] = seg[3][i] + n_out; seg[5][i + 1] = seg[5][i] + (n_out + kTempoHop - 1) / kTempoHop;
    }
    return seg[5][count];
}
TempoArgs tempo_args(bark_context * c, const int (&seg)[6][kResampleMaxSegments + 1], int count) {
    c->tp_in.reserve(c, (size_t) seg[1][count]);
    c->tp_out.reserve(c, (size_t) seg[3][count]);
    c->tp_pos.reserve(c, (size_t) seg[5][count]);
    c->tp_seg.reserve(c, 6 * (kResampleMaxSegments + 1));
    if (!c->tp_win_ready) {
        c->tp_win.reserve(c, (size_t) kTempoFrame);
        HIP_OK(hipMemcpyAsync(c->tp_win.p, tempo_window(), kTempoFrame * sizeof(float), hipMemcpyHostToDevice, c->stream));
        HIP_OK(hipStreamSynchronize(c->stream));
        c->tp_win_ready = true;
    }
    TempoArgs a;
    a.x = c->tp_in.p; a.y = c->tp_out.p; a.win = c->tp_win.p; a.seg = c->tp_seg.p; a.pos = c->tp_pos.p; a.B = count;
    return a;
}
std::vector<uint8_t> tempo_staged(bark_context * c, const TempoArgs & a, const int (&seg)[6][kResampleMaxSegments + 1], int count, int rate_out, int fmt,
                                  std::vector<int32_t> & n_out, std::vector<int32_t> * positions);
}  // namespace

std::vector<uint8_t> engine_tempo_many(bark_context * c, const float * const * pcm, const int * n, int count, const int32_t * speed, int rate_out, int fmt,
                                       std::vector<int32_t> & n_out, std::vector<int32_t> * positions) {
    HIP_OK(hipSetDevice(c->device));
    if (!pcm || !n || !speed || count < 1 || count > kResampleMaxSegments) throw std::runtime_error("tempo: 1 .. 64 segments in one call");
    if (!resample_pair_supported(24000, rate_out)) throw std::runtime_error("tempo: the rates are 8000, 12000, 16000, 22050, 24000, 32000, 44100 and 48000");
    const int bytes_per = render_format_bytes(fmt);
    if (!bytes_per) throw std::runtime_error("tempo: the sample formats are f32 (0), s16 (1), mu-law (2) and FLAC (3)");
    bool all_identity = true;
    for (int i = 0; i < count; i++) {
        if (!pcm[i] || tempo_out_len(n[i], speed[i]) < 0) throw std::runtime_error("tempo: a segment needs 1 .. 1 310 720 samples and a speed of 500 .. 2000 per mille");
        for (int k = 0; k < n[i]; k++) if (!(std::fabs(pcm[i][k]) < 65520.0f)) throw std::runtime_error("tempo: a sample that is not finite or not below 65520 in magnitude");
        all_identity = all_identity && speed[i] == 1000;
    }
    if (all_identity && !positions) return engine_resample_many(c, pcm, n, count, 24000, rate_out, fmt, n_out);      // nothing of the rule runs
    int seg[6][kResampleMaxSegments + 1];
    fill_tempo_table(seg, n, speed, count);
    const TempoArgs a = tempo_args(c, seg, count);
    for (int i = 0; i < count; i++) HIP_OK(hipMemcpyAsync(c->tp_in.p + seg[1][i], pcm[i], (size_t) n[i] * 4, hipMemcpyHostToDevice, c->stream));
    return tempo_staged(c, a, seg, count, rate_out, fmt, n_out, positions);
}

namespace {
// the device half of engine_tempo_many: the segments lie back to back in tp_in
std::vector<uint8_t> tempo_staged(bark_context * c, const TempoArgs & a, const int (&seg)[6][kResampleMaxSegments + 1], int count, int rate_out, int fmt,
                                  std::vector<int32_t> & n_out, std::vector<int32_t> * positions) {
    const int bytes_per = render_format_bytes(fmt), n_frames = seg[5][count];
    hipStream_t s = c->stream;
    HIP_OK(hipMemcpyAsync(c->tp_seg.p, seg, sizeof(seg), hipMemcpyHostToDevice, s));
    launch_tempo(s, a, seg);
    if (positions) {
        positions->assign((size_t) n_frames, 0);
        HIP_OK(hipMemcpyAsync(positions->data(), c->tp_pos.p, (size_t) n_frames * 4, hipMemcpyDeviceToHost, s));
    }
    const ResampleTable * t = resample_pair_table(24000, rate_out);
    std::vector<uint8_t> out;
    if (!t && fmt == BARK_HIP_SAMPLE_F32) {                      // 24 kHz f32: the time-scaled samples themselves
        n_out.assign(seg[2], seg[2] + count);
        out.resize((size_t) seg[3][count] * 4);
        HIP_OK(hipMemcpyAsync(out.data(), c->tp_out.p, out.size(), hipMemcpyDeviceToHost, s));
        HIP_OK(hipStreamSynchronize(s));                         // seg is a stack object
        return out;
    }
    int rseg[5][kResampleMaxSegments + 1];
    const int n_tiles = fill_segment_table(rseg, seg[2], count, 24000, rate_out, n_out);
    out.resize((size_t) rseg[3][count] * (size_t) bytes_per);
    c->rp_out.reserve(c, out.size());
    c->rp_seg.reserve(c, 5 * (kResampleMaxSegments + 1));
    convert_staged(c, c->tp_out.p, rseg, n_tiles, count, (size_t) seg[3][count], t, 24000, rate_out, fmt, out);
    return out;
}
}  // namespace

// ---- loudness (rule C17l) ----------------------------------------------------------------------------------------------------------------------------------
bool loudness_params_valid(const bark_hip_loudness_params & p) {
    return (p.target_centilufs == 0 || (p.target_centilufs >= kLoudMinTarget && p.target_centilufs <= kLoudMaxTarget)) &&
           std::isfinite(p.peak_ceiling) && p.peak_ceiling >= 0.0f && std::isfinite(p.max_gain) && p.max_gain >= 0.0f;
}
double loudness_target_ms(int t) { return std::pow(10.0, ((double) t / 100.0 + 0.691) / 10.0); }
namespace {
// the segment table of launch_loudness_hops
void fill_loudness_table(int (&seg)[5][kResampleMaxSegments + 1], const int * n, int count) {
    memset(seg, 0, sizeof(seg));
    for (int i = 0; i < count; i++) {
        const int Hn = n[i] / kLoudHop;
        seg[0][i] = n[i]; seg[2][i] = Hn;
        seg[1][i + 1] = seg[1][i] + n[i]; seg[3][i + 1] = seg[3][i] + Hn; seg[4][i + 1] = seg[4][i] + Hn + 1;
    }
}
LoudnessArgs loudness_args(bark_context * c, const int (&seg)[5][kResampleMaxSegments + 1], int count) {
    c->lv_in.reserve(c, (size_t) seg[1][count]);
    c->lv_z.reserve(c, (size_t) std::max(seg[3][count], 1));
    c->lv_seg.reserve(c, 5 * (kResampleMaxSegments + 1));
    c->lv_peak.reserve(c, (size_t) kResampleMaxSegments);
    c->lv_req.reserve(c, (size_t) kResampleMaxSegments);
    c->lv_info.reserve(c, (size_t) kResampleMaxSegments);
    LoudnessArgs a;
    a.x = c->lv_in.p; a.seg = c->lv_seg.p; a.z = c->lv_z.p; a.peak = c->lv_peak.p; a.req = c->lv_req.p; a.info = c->lv_info.p; a.B = count;
    return a;
}
void loudness_check(const float * const * pcm, const int * n, int count, const bark_hip_loudness_params * params) {
    if (!pcm || !n || count < 1 || count > kResampleMaxSegments) throw std::runtime_error("loudness: 1 .. 64 segments in one call");
    for (int i = 0; i < count; i++) {
        if (!pcm[i] || n[i] < 1 || n[i] > kResampleMaxSamples) throw std::runtime_error("loudness: a segment needs 1 .. 1 310 720 samples");
        if (params && !loudness_params_valid(params[i])) throw std::runtime_error("loudness: a target of -40 .. -5 LUFS (or 0: off), a ceiling and a cap that are >= 0 and finite");
        for (int k = 0; k < n[i]; k++) if (!(std::fabs(pcm[i][k]) < 65520.0f)) throw std::runtime_error("loudness: a sample that is not finite or not below 65520 in magnitude");
    }
}
// upload, measure, level: a.y (may be null) receives the levelled samples; `info` and (if wanted) `z` are read back behind the caller's next synchronisation
void loudness_run(bark_context * c, LoudnessArgs a, const int (&seg)[5][kResampleMaxSegments + 1], const float * const * pcm, const int * n, int count,
                  const bark_hip_loudness_params * params, LoudnessInfo (&info)[kResampleMaxSegments], std::vector<double> * z) {
    hipStream_t s = c->stream;
    LoudnessReq req[kResampleMaxSegments];
    for (int i = 0; i < count; i++)
        if (params && params[i].target_centilufs != 0) { req[i].tms = loudness_target_ms(params[i].target_centilufs); req[i].max_gain = params[i].max_gain; req[i].peak_ceiling = params[i].peak_ceiling; }
    for (int i = 0; i < count; i++) HIP_OK(hipMemcpyAsync(c->lv_in.p + seg[1][i], pcm[i], (size_t) n[i] * 4, hipMemcpyHostToDevice, s));
    HIP_OK(hipMemcpyAsync(c->lv_seg.p, seg, sizeof(seg), hipMemcpyHostToDevice, s));
    HIP_OK(hipMemcpyAsync(c->lv_req.p, req, sizeof(LoudnessReq) * (size_t) count, hipMemcpyHostToDevice, s));
    HIP_OK(hipMemsetAsync(c->lv_peak.p, 0, sizeof(unsigned) * (size_t) count, s));
    launch_loudness_hops(s, a, seg);
    launch_loudness_level(s, a);
    HIP_OK(hipMemcpyAsync(info, c->lv_info.p, sizeof(LoudnessInfo) * (size_t) count, hipMemcpyDeviceToHost, s));
    if (z) {
        z->assign((size_t) seg[3][count], 0.0);
        if (!z->empty()) HIP_OK(hipMemcpyAsync(z->data(), c->lv_z.p, z->size() * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    HIP_OK(hipStreamSynchronize(s));                             // req is a stack object; a later launch on the stream still reads a.y in order
}
std::vector<bark_hip_loudness_info> public_info(const LoudnessInfo * info, int count) {
    std::vector<bark_hip_loudness_info> out((size_t) count);
    for (int i = 0; i < count; i++) {
        bark_hip_loudness_info & o = out[(size_t) i];
        o.mean_square = info[i].mean_square;
        o.lufs = info[i].mean_square > 0.0 ? -0.691 + 10.0 * std::log10(info[i].mean_square) : -INFINITY;       // for information: the host's log10
        o.peak = info[i].peak; o.gain = info[i].gain; o.n_blocks = info[i].n_blocks; o.n_abs = info[i].n_abs; o.n_gated = info[i].n_gated; o.flags = info[i].flags;
    }
    return out;
}
}  // namespace

std::vector<bark_hip_loudness_info> engine_loudness_many(bark_context * c, const float * const * pcm, const int * n, int count, const bark_hip_loudness_params * params,
                                                         std::vector<double> * z) {
    HIP_OK(hipSetDevice(c->device));
    loudness_check(pcm, n, count, params);
    int seg[5][kResampleMaxSegments + 1];
    fill_loudness_table(seg, n, count);
    const LoudnessArgs a = loudness_args(c, seg, count);
    LoudnessInfo info[kResampleMaxSegments];
    loudness_run(c, a, seg, pcm, n, count, params, info, z);
    return public_info(info, count);
}

std::vector<uint8_t> engine_level_many(bark_context * c, const float * const * pcm, const int * n, int count, const bark_hip_loudness_params * params,
                                       const int32_t * speed, int rate_out, int fmt, std::vector<int32_t> & n_out, std::vector<bark_hip_loudness_info> * info_out) {
    HIP_OK(hipSetDevice(c->device));
    if (!params || !speed) throw std::runtime_error("level: a request and a speed per segment");
    loudness_check(pcm, n, count, params);
    if (!resample_pair_supported(24000, rate_out)) throw std::runtime_error("level: the rates are 8000, 12000, 16000, 22050, 24000, 32000, 44100 and 48000");
    const int bytes_per = render_format_bytes(fmt);
    if (!bytes_per) throw std::runtime_error("level: the sample formats are f32 (0), s16 (1), mu-law (2) and FLAC (3)");
    bool all_off = true, all_identity = true;
    for (int i = 0; i < count; i++) {
        if (tempo_out_len(n[i], speed[i]) < 0) throw std::runtime_error("level: a speed of 500 .. 2000 per mille");
        all_off = all_off && params[i].target_centilufs == 0;
        all_identity = all_identity && speed[i] == 1000;
    }
    if (all_off) {                                               // nothing of the rule runs
        if (info_out) { bark_hip_loudness_info one{}; one.gain = 1.0f; info_out->assign((size_t) count, one); }
        return engine_tempo_many(c, pcm, n, count, speed, rate_out, fmt, n_out);
    }
    int seg[5][kResampleMaxSegments + 1];
    fill_loudness_table(seg, n, count);
    LoudnessArgs a = loudness_args(c, seg, count);
    LoudnessInfo info[kResampleMaxSegments];
    const size_t total_in = (size_t) seg[1][count];
    std::vector<uint8_t> out;
    if (!all_identity) {                                         // the levelled samples are the tempo kernel's input
        int tseg[6][kResampleMaxSegments + 1];
        fill_tempo_table(tseg, n, speed, count);
        const TempoArgs ta = tempo_args(c, tseg, count);
        a.y = c->tp_in.p;
        loudness_run(c, a, seg, pcm, n, count, params, info, nullptr);
        out = tempo_staged(c, ta, tseg, count, rate_out, fmt, n_out, nullptr);
    } else {                                                     // .. or the resampler's
        int rseg[5][kResampleMaxSegments + 1];
        const int n_tiles = fill_segment_table(rseg, n, count, 24000, rate_out, n_out);
        out.resize((size_t) rseg[3][count] * (size_t) bytes_per);
        ensure_resample_buffers(c, total_in, out.size());
        a.y = c->rp_in.p;
        loudness_run(c, a, seg, pcm, n, count, params, info, nullptr);
        const ResampleTable * t = resample_pair_table(24000, rate_out);
        if (!t && fmt == BARK_HIP_SAMPLE_F32) {                  // 24 kHz f32: the levelled samples themselves
            HIP_OK(hipMemcpyAsync(out.data(), c->rp_in.p, out.size(), hipMemcpyDeviceToHost, c->stream));
            HIP_OK(hipStreamSynchronize(c->stream));
        } else convert_staged(c, c->rp_in.p, rseg, n_tiles, count, total_in, t, 24000, rate_out, fmt, out);
    }
    if (info_out) *info_out = public_info(info, count);
    return out;
}

double engine_time_loudness(bark_context * c, int count, int n_each, int iters, bool level) {
    HIP_OK(hipSetDevice(c->device));
    if (count < 1 || count > kResampleMaxSegments || n_each < 1 || n_each > kResampleMaxSamples) throw std::runtime_error("time_loudness: 1 .. 64 segments of 1 .. 1 310 720 samples");
    const std::vector<int> n((size_t) count, n_each);
    int seg[5][kResampleMaxSegments + 1];
    fill_loudness_table(seg, n.data(), count);
    LoudnessArgs a = loudness_args(c, seg, count);
    c->rp_in.reserve(c, (size_t) seg[1][count]);
    a.y = c->rp_in.p;
    LoudnessReq req[kResampleMaxSegments];
    for (int i = 0; i < count; i++) { req[i].tms = loudness_target_ms(-1600); req[i].max_gain = 10.0f; req[i].peak_ceiling = 1.0f; }
    hipStream_t s = c->stream;
    HIP_OK(hipMemsetAsync(c->lv_in.p, 0, (size_t) seg[1][count] * 4, s));      // the time does not depend on the values: every chain runs in full
    HIP_OK(hipMemcpyAsync(c->lv_seg.p, seg, sizeof(seg), hipMemcpyHostToDevice, s));
    HIP_OK(hipMemcpyAsync(c->lv_req.p, req, sizeof(LoudnessReq) * (size_t) count, hipMemcpyHostToDevice, s));
    HIP_OK(hipMemsetAsync(c->lv_peak.p, 0, sizeof(unsigned) * (size_t) count, s));
    HIP_OK(hipStreamSynchronize(s));
    iters = std::max(1, iters);
    launch_loudness_hops(s, a, seg);                             // the level launch reads what a hops launch wrote
    auto one = [&] { if (level) launch_loudness_level(s, a); else launch_loudness_hops(s, a, seg); };
    for (int i = 0; i < 2; i++) one();
    return time_on_stream_us(c, [&] { for (int i = 0; i < iters; i++) one(); }) / iters;
}

// ---- FLAC (rule C18f) --------------------------------------------------------------------------------------------------------------------------------------
long long flac_max_bytes(long long n) {
    if (n < 1 || n > kFlacMaxSamples) return -1;
    return kFlacStreamHeader + kFlacFrameOverhead * ((n + kFlacBlock - 1) / kFlacBlock) + 2 * n;
}
namespace {
// the segment table of launch_flac_frames; returns the frame count, or -1 where the samples or the frames would not fit the kernels' int offsets
long long fill_flac_table(int (&seg)[3][kResampleMaxSegments + 1], const int * n, int count) {
    memset(seg, 0, sizeof(seg));
    long long samples = 0, frames = 0;
    for (int i = 0; i < count; i++) {
        samples += n[i]; frames += (n[i] + kFlacBlock - 1) / kFlacBlock;
        if (samples > (1LL << 30)) return -1;
        seg[0][i] = n[i]; seg[1][i + 1] = (int) samples; seg[2][i + 1] = (int) frames;
    }
    return frames;
}
// the marker and the STREAMINFO block, marked last: block sizes 4096 and 4096, the smallest and the largest frame, rate, one channel, 16 bits, the sample
// count, and an MD5 field of zeros (not computed)
void flac_stream_header(uint8_t * h, long long n, int rate, int min_frame, int max_frame) {
    memset(h, 0, kFlacStreamHeader);
    memcpy(h, "fLaC", 4);
    h[4] = 0x80; h[7] = 34;
    h[8] = kFlacBlock >> 8; h[9] = kFlacBlock & 0xFF; h[10] = kFlacBlock >> 8; h[11] = kFlacBlock & 0xFF;
    h[12] = (uint8_t) (min_frame >> 16); h[13] = (uint8_t) (min_frame >> 8); h[14] = (uint8_t) min_frame;
    h[15] = (uint8_t) (max_frame >> 16); h[16] = (uint8_t) (max_frame >> 8); h[17] = (uint8_t) max_frame;
    const uint64_t v = ((uint64_t) rate << 44) | ((uint64_t) 15 << 36) | (uint64_t) n;        // 20 bits of rate, channels - 1 = 0, bits - 1 = 15, 36 bits of samples
    for (int i = 0; i < 8; i++) h[18 + i] = (uint8_t) (v >> (56 - 8 * i));
}
FlacArgs flac_args(bark_context * c, const int16_t * dx, int count, long long frames, long long samples, int rate) {
    c->fl_seg.reserve(c, 3 * (kResampleMaxSegments + 1));
    c->fl_scratch.reserve(c, (size_t) frames * (kFlacFrameStride / 4) + 4);       // the pack kernel reads whole words: one beyond the last frame's bytes
    c->fl_len.reserve(c, (size_t) frames);
    c->fl_info.reserve(c, (size_t) frames * 4);
    c->fl_tot.reserve(c, 3 * (size_t) kResampleMaxSegments);
    c->fl_out.reserve(c, (size_t) (frames * kFlacFrameOverhead + 2 * samples) + 4);
    FlacArgs a;
    a.x = dx; a.seg = c->fl_seg.p; a.scratch = c->fl_scratch.p; a.flen = c->fl_len.p; a.finfo = c->fl_info.p; a.out = c->fl_out.p; a.tot = c->fl_tot.p;
    a.B = count; a.rate_code = flac_rate_code(rate); a.rate_khz = rate / 1000;
    return a;
}
// the workgroups that share a result's copy in the pack launch: one per 4 frames of the longest result, at most 64 (one workgroup copying the 30 frames
// of a 5.12 s result alone took 45 us)
int flac_pack_split(const int (&seg)[3][kResampleMaxSegments + 1], int count) {
    int most = 1;
    for (int i = 0; i < count; i++) most = std::max(most, seg[2][i + 1] - seg[2][i]);
    return std::min(64, (most + 3) / 4);
}
std::vector<uint8_t> flac_staged(bark_context * c, const int16_t * dx, const int * n, int count, int rate, std::vector<int32_t> & lengths, std::vector<int32_t> * frames_out) {
    if (!flac_rate_code(rate)) throw std::runtime_error("flac: the rates are 8000, 12000, 16000, 22050, 24000, 32000, 44100 and 48000");
    int seg[3][kResampleMaxSegments + 1];
    const long long frames = fill_flac_table(seg, n, count);
    if (frames < 0) throw std::runtime_error("flac: more than 2^30 samples in one call");
    const FlacArgs a = flac_args(c, dx, count, frames, seg[1][count], rate);
    hipStream_t s = c->stream;
    HIP_OK(hipMemcpyAsync(c->fl_seg.p, seg, sizeof(seg), hipMemcpyHostToDevice, s));
    launch_flac_frames(s, a, seg);
    launch_flac_pack(s, a, flac_pack_split(seg, count));
    int tot[3][kResampleMaxSegments];
    HIP_OK(hipMemcpyAsync(tot, c->fl_tot.p, sizeof(tot), hipMemcpyDeviceToHost, s));
    if (frames_out) {
        frames_out->assign((size_t) frames * 4, 0);
        HIP_OK(hipMemcpyAsync(frames_out->data(), c->fl_info.p, frames_out->size() * 4, hipMemcpyDeviceToHost, s));
    }
    HIP_OK(hipStreamSynchronize(s));                             // the totals size the copy below; seg is a stack object
    size_t packed = 0;
    for (int i = 0; i < count; i++) packed += (size_t) tot[0][i];
    if (packed > c->fl_out.n) throw std::runtime_error("flac: the device reports more bytes than the bound");
    std::vector<uint8_t> body(packed);
    HIP_OK(hipMemcpyAsync(body.data(), c->fl_out.p, packed, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    std::vector<uint8_t> out(packed + (size_t) count * kFlacStreamHeader);
    lengths.assign((size_t) count, 0);
    size_t at = 0, from = 0;
    for (int i = 0; i < count; i++) {
        flac_stream_header(out.data() + at, n[i], rate, tot[1][i], tot[2][i]);
        memcpy(out.data() + at + kFlacStreamHeader, body.data() + from, (size_t) tot[0][i]);
        lengths[(size_t) i] = kFlacStreamHeader + tot[0][i];
        at += (size_t) lengths[(size_t) i]; from += (size_t) tot[0][i];
    }
    return out;
}
}  // namespace

std::vector<uint8_t> engine_flac_encode_many(bark_context * c, const int16_t * const * pcm, const int * n, int count, int rate, std::vector<int32_t> & lengths,
                                             std::vector<int32_t> * frames) {
    HIP_OK(hipSetDevice(c->device));
    if (!pcm || !n || count < 1 || count > kResampleMaxSegments) throw std::runtime_error("flac: 1 .. 64 results in one call");
    if (!flac_rate_code(rate)) throw std::runtime_error("flac: the rates are 8000, 12000, 16000, 22050, 24000, 32000, 44100 and 48000");
    long long samples = 0;
    for (int i = 0; i < count; i++) {
        if (!pcm[i] || flac_max_bytes(n[i]) < 0) throw std::runtime_error("flac: a result needs 1 .. 2^26 samples");
        samples += n[i];
    }
    if (samples > (1LL << 30)) throw std::runtime_error("flac: more than 2^30 samples in one call");
    c->fl_in.reserve(c, (size_t) samples);
    size_t off = 0;
    for (int i = 0; i < count; i++) { HIP_OK(hipMemcpyAsync(c->fl_in.p + off, pcm[i], (size_t) n[i] * 2, hipMemcpyHostToDevice, c->stream)); off += (size_t) n[i]; }
    return flac_staged(c, c->fl_in.p, n, count, rate, lengths, frames);
}

double engine_time_flac(bark_context * c, int count, int n_each, int iters, int which) {
    HIP_OK(hipSetDevice(c->device));
    if (count < 1 || count > kResampleMaxSegments || n_each < 1 || n_each > kResampleMaxSamples) throw std::runtime_error("time_flac: 1 .. 64 results of 1 .. 1 310 720 samples");
    // the time depends on the values (the codes' lengths): a voiced tone under a slow envelope with a little noise on top, the same for every result
    std::vector<int16_t> x((size_t) n_each);
    uint32_t lcg = 12345u;
    for (int i = 0; i < n_each; i++) {
        lcg = lcg * 1664525u + 1013904223u;
        const double env = 0.5 + 0.5 * sin(2.0 * M_PI * 3.0 * i / 24000.0);
        x[(size_t) i] = (int16_t) lround(6000.0 * env * sin(2.0 * M_PI * 220.0 * i / 24000.0) + 1500.0 * env * sin(2.0 * M_PI * 1870.0 * i / 24000.0) + (double) ((int) (lcg >> 25) - 64));
    }
    const std::vector<int> n((size_t) count, n_each);
    int seg[3][kResampleMaxSegments + 1];
    const long long frames = fill_flac_table(seg, n.data(), count);
    c->fl_in.reserve(c, (size_t) count * (size_t) n_each);
    const FlacArgs a = flac_args(c, c->fl_in.p, count, frames, seg[1][count], 24000);
    hipStream_t s = c->stream;
    for (int i = 0; i < count; i++) HIP_OK(hipMemcpyAsync(c->fl_in.p + (size_t) i * (size_t) n_each, x.data(), x.size() * 2, hipMemcpyHostToDevice, s));
    HIP_OK(hipMemcpyAsync(c->fl_seg.p, seg, sizeof(seg), hipMemcpyHostToDevice, s));
    HIP_OK(hipStreamSynchronize(s));
    const int split = flac_pack_split(seg, count);
    iters = std::max(1, iters);
    launch_flac_frames(s, a, seg);                               // the pack launch reads what a frames launch wrote
    auto one = [&] { if (which != 2) launch_flac_frames(s, a, seg); if (which != 1) launch_flac_pack(s, a, split); };
    for (int i = 0; i < 2; i++) one();
    return time_on_stream_us(c, [&] { for (int i = 0; i < iters; i++) one(); }) / iters;
}

double engine_time_tempo(bark_context * c, int count, int n_each, int speed, int iters) {
    HIP_OK(hipSetDevice(c->device));
    if (count < 1 || count > kResampleMaxSegments || tempo_out_len(n_each, speed) < 0 || speed == 1000)
        throw std::runtime_error("time_tempo: 1 .. 64 segments of 1 .. 1 310 720 samples at 500 .. 2000 per mille, not 1000 (which runs no search)");
    const std::vector<int> n((size_t) count, n_each);
    const std::vector<int32_t> sp((size_t) count, speed);
    int seg[6][kResampleMaxSegments + 1];
    fill_tempo_table(seg, n.data(), sp.data(), count);
    const TempoArgs a = tempo_args(c, seg, count);
    HIP_OK(hipMemsetAsync(c->tp_in.p, 0, (size_t) count * (size_t) n_each * 4, c->stream));       // the time does not depend on the values: every chain runs in full
    HIP_OK(hipMemcpyAsync(c->tp_seg.p, seg, sizeof(seg), hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    iters = std::max(1, iters);
    for (int i = 0; i < 2; i++) launch_tempo(c->stream, a, seg);
    return time_on_stream_us(c, [&] { for (int i = 0; i < iters; i++) launch_tempo(c->stream, a, seg); }) / iters;
}

// ---- long-form text: split (C15s), run the chunks as lock-step jobs, keep the results for the join (C15j) -------------------------------------------------
int engine_generate_long(bark_context * c, const char * text, const bark_hip_long_params & lp, const bark_hip_request_params * rp, const bark_hip_sampling_filter * flt,
                         const VoicePtr * voice) {
    c->long_result = bark_context::LongResult();                        // a refused or failed call leaves no result behind
    if (lp.chain != 0 && lp.chain != 1) throw std::runtime_error("generate_long: chain is 0 (one job) or 1 (every chunk continues the one before it)");
    if (!join_params_valid(lp.join)) throw std::runtime_error("generate_long: gap_samples >= 0, fade_samples 0 .. 24000, trim_threshold >= 0 and finite, trim_pad_frames >= 0");
    const std::string full(text);
    std::vector<TextSpan> spans = split_text(c->vocab, full, lp.max_tokens);
    if (spans.empty()) spans.push_back({0, (int32_t) full.size()});      // a text without a word runs as one chunk, as it does today
    const int n = (int) spans.size();
    const bark_context_params & p = c->params;
    bark_hip_request_params base = rp ? *rp : bark_hip_request_params{p.temp, p.fine_temp, p.min_eos_p, p.n_steps_text_encoder, (uint32_t) c->rng()};
    std::vector<std::string> texts;
    std::vector<const char *> ptrs;
    std::vector<bark_hip_request_params> rps((size_t) n, base);
    for (int i = 0; i < n; i++) {
        texts.push_back(full.substr((size_t) spans[(size_t) i].begin, (size_t) (spans[(size_t) i].end - spans[(size_t) i].begin)));
        rps[(size_t) i].seed = base.seed + (uint32_t) i;                 // wraps in uint32
    }
    for (const std::string & t : texts) ptrs.push_back(t.c_str());
    const std::vector<bark_hip_sampling_filter> flts((size_t) n, flt ? *flt : c->filter);
    bark_context::LongResult res;
    res.spans = spans; res.join = lp.join;
    if (lp.chain == 0) {
        const std::vector<VoicePtr> voices((size_t) n, voice ? *voice : VoicePtr());
        if (engine_generate_batch(c, ptrs.data(), n, nullptr, rps.data(), nullptr, flts.data(), voices.data()) != n) throw std::runtime_error("generate_long: a chunk failed");
        res.chunks = c->batch_results;
    } else {
        VoicePtr v = voice ? *voice : VoicePtr();
        for (int i = 0; i < n; i++) {
            if (engine_generate_batch(c, &ptrs[(size_t) i], 1, nullptr, &rps[(size_t) i], nullptr, &flts[(size_t) i], &v) != 1) throw std::runtime_error("generate_long: a chunk failed");
            res.chunks.push_back(c->batch_results[0]);
            const bark_context::BatchResult & r = res.chunks.back();
            const bark_hip_voice_prompt vp{r.semantic.data(), (int32_t) r.semantic.size(), r.coarse.data(), (int32_t) (r.coarse.size() / 2), r.fine.data(), (int32_t) (r.fine.size() / 8)};
            try { v = engine_make_voice(c, &vp); } catch (const std::exception &) {}          // a history too short to continue from: the next chunk keeps this one's voice
        }
    }
    for (const bark_context::BatchResult & r : res.chunks) if (!r.ok || r.audio.empty() || r.audio.size() > (size_t) kResampleMaxSamples) throw std::runtime_error("generate_long: a chunk gave no audio");
    c->long_result = std::move(res);
    return n;
}

VoicePtr engine_voice_from_audio(bark_context * c, const float * pcm, int n) {
    if (!c->hub) throw std::runtime_error("voice from audio: no semantic encoder loaded (bark_hip_load_semantic_encoder)");
    if (!c->codec.enc.present) throw std::runtime_error("voice from audio: the model file holds no codec encoder");
    if (!pcm || n < 599) throw std::runtime_error("voice from audio: a recording needs at least 599 samples (400 at 16 kHz: one semantic frame)");
    // every sample is looked at, also those in front of the part that is used: a recording with a hole in it is refused as a whole
    for (int i = 0; i < n; i++) if (!std::isfinite(pcm[i]) || !std::isfinite((float) (_Float16) pcm[i])) throw std::runtime_error("voice from audio: non-finite sample (or one beyond the f16 range)");
    if (n > kVoiceAudioMaxSamples) { pcm += n - kVoiceAudioMaxSamples; n = kVoiceAudioMaxSamples; }      // every stage reads the END of its history stream
    const std::vector<float> x16 = engine_resample_24k_16k(c, pcm, n);
    const std::vector<int32_t> sem = engine_semantic_encode(c, x16.data(), (int) x16.size(), -1, nullptr);
    const std::vector<int32_t> codes = std::move(engine_codec_encode_many(c, {pcm}, {n}, 8, -1, nullptr)[0]);      // [8][T]
    const int T = (int) (codes.size() / 8);
    std::vector<int32_t> coarse((size_t) T * 2), fine((size_t) T * 8);
    for (int t = 0; t < T; t++) for (int q = 0; q < 8; q++) {
        fine[(size_t) t * 8 + q] = codes[(size_t) q * T + t];
        if (q < 2) coarse[(size_t) t * 2 + q] = codes[(size_t) q * T + t];
    }
    const bark_hip_voice_prompt v{sem.data(), (int32_t) sem.size(), coarse.data(), T, fine.data(), T};
    return engine_make_voice(c, &v);
}

}  // namespace barkhip
