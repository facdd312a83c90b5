// codec_kernels.hip - EnCodec 24 kHz decoder kernels (RVQ de-embedding, SEANet conv / LSTM /
// transposed-conv stack).  Architecture restated from HF transformers modeling_encodec.py:82-450 (the
// model the reference's convert.py converts from; the reference delegates this stage to the
// un-vendored encodec.cpp, call site /root/reference/bark.cpp:2143-2167).
// Activations are TIME-MAJOR [row][C] (row = frame of the stage; the utterances of a batch back to back: utterance b owns rows
// [tm Tpre[b], tm Tpre[b + 1]) at a stage with upsampling factor tm), so that a convolution is a product on the f16 matrix cores: order
// C9m = the arithmetic of v_mfma_f32_32x32x16_f16 (oracle/mfma_f16_emu.h) over the axis kd = k * cin + ci (transposed conv: one product
// per output phase over tap * cin + ci).  Convolutions whose input channel count is not a multiple of 8 (toy models) keep order C9 (one fmaf
// chain in (ci, k) order) in a plain kernel; BARK_HIP_CROSSCHECK bit 10 (1024) sends every convolution there (oracle: set_codec_mfma(False)).
// Every kernel takes a CodecBatch: the codec of a lock-step batch costs the launches of ONE utterance.
// At the end of the file: the semantic encoder's own kernels (rule C12h) - convolution 0 with its norm over time and the grouped positional convolution;
// its six strided convolutions are the valid mode of conv_down_*_kernel.
#include "kernels.h"

namespace barkhip {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));

// utterance blockIdx.z of a batch: its frame count (times the stage's upsampling factor) and the element offsets of its input / output arrays
struct UttView { int T; size_t in_off, out_off; };
__device__ __forceinline__ UttView utt_view(const CodecBatch & cb, int T, int tmul_in, int tmul_out, int cin, int cout) {
    if (!cb.T) return UttView{T, 0, 0};
    const int z = blockIdx.z;
    return UttView{cb.T[z] * tmul_in, (size_t) cin * tmul_in * cb.Tpre[z], (size_t) cout * tmul_out * cb.Tpre[z]};
}

// first row of the utterance that owns global row `row` at upsampling factor tm, and that utterance's row count
__device__ __forceinline__ void utt_of_row(const CodecBatch & cb, int T_single, int tm, int row, int & row0, int & rows) {
    if (!cb.T) { row0 = 0; rows = T_single * tm; return; }
    int z = 0;
    while (z + 1 < cb.B && row >= cb.Tpre[z + 1] * tm) z++;
    row0 = cb.Tpre[z] * tm; rows = cb.T[z] * tm;
}

// z[frame][h] = 0 + sum_q embed_q[code] (modeling_encodec.py:440-448); codes of utterance b: [n_q][T[b]] at n_q Tpre[b]
__global__ void rvq_gather_kernel(const float * codebooks, int n_bins, int Hd, const int32_t * codes, int n_q, int T_, int rows_total, float * z, const CodecBatch cb) {
    const int row = blockIdx.x;
    if (row >= rows_total) return;
    int row0, rows;
    utt_of_row(cb, T_, 1, row, row0, rows);
    const int32_t * cz = codes + (size_t) n_q * row0;
    const int t = row - row0;
    for (int d = threadIdx.x; d < Hd; d += blockDim.x) {
        float v = 0.0f;
        for (int q = 0; q < n_q; q++) {
            int id = cz[(size_t) q * rows + t];
            id = min(max(id, 0), n_bins - 1);
            v = v + codebooks[((size_t) q * n_bins + id) * Hd + d];
        }
        z[(size_t) row * Hd + d] = v;
    }
}
void launch_rvq_gather(hipStream_t s, const float * codebooks, int n_bins, int Hd, const int32_t * codes, int n_q, int T, int rows_total, float * z, const CodecBatch & cb) {
    hipLaunchKernelGGL(rvq_gather_kernel, dim3(rows_total), dim3(128), 0, s, codebooks, n_bins, Hd, codes, n_q, T, rows_total, z, cb);
}

// see kernels.hip: keeps the compiler from fusing the producing multiply into the f16 conversion
__device__ __forceinline__ half_t to_half(float v) { asm("" : "+v"(v)); return (half_t) v; }
__device__ __forceinline__ float elu_canon(float x) { return x > 0.0f ? x : (float) expm1((double) x); }

__global__ void act_round_kernel(const float * x, size_t n, int elu, half_t * out) {
    for (size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t) gridDim.x * blockDim.x) {
        float v = x[i];
        if (elu) v = elu_canon(v);
        out[i] = to_half(v);
    }
}
void launch_act_round(hipStream_t s, const float * x, size_t n, int elu, half_t * out_h) {
    const int blocks = (int) ((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(act_round_kernel, dim3(blocks), dim3(256), 0, s, x, n, elu, out_h);
}

// EncodecConv1d: causal, stride 1, pad_mode reflect (modeling_encodec.py:140-176): left pad K - 1; the reflect source of padded index
// i < left is x[left - i]; inputs shorter than the pad are zero-extended first.
// EncodecConvTranspose1d, causal, kernel 2 s: full output (T - 1) s + K trimmed by K - s on the right (modeling_encodec.py:206-233):
// output row q s + r takes frame q - 1 through kernel element r + s and frame q through element r.
// source row of tap kk for the output built from input row t of an utterance of `rows` rows; -1: the operand is zero
__device__ __forceinline__ int conv_src_row(int convT, int K, int kk, int t, int rows) {
    int j;
    if (convT) j = t - 1 + kk;                                    // tap 0: the previous frame, tap 1: this frame
    else { j = t + kk - (K - 1); j = j < 0 ? -j : j; }            // reflect on the left
    return (j >= 0 && j < rows) ? j : -1;
}

// C9m: one wave = 32 input rows x 32 output channels of one output phase; A = kernel image rows (co), B = activation rows (time), both
// 8 consecutive kd per lane = one 16-byte load; the accumulator walks kd in ascending blocks of 16 - the canonical chain.
typedef float floatx16c __attribute__((ext_vector_type(16)));
__global__ __launch_bounds__(256) void conv_tm_mfma_kernel(const ConvTmArgs a) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, half = lane >> 5, l31 = lane & 31;
    const int row = (blockIdx.x * 4 + w) * 32 + l31;              // global input row of this lane's column
    const int co0 = blockIdx.y * 32, phase = blockIdx.z;
    const bool live = row < a.rows_in;
    int row0 = 0, rows = 0;
    if (live) utt_of_row(a.cb, a.T_single, a.tm_in, row, row0, rows);
    const int t = row - row0;
    const int nkb = a.kd16 >> 4;
    const half_t * wrow = a.W + ((size_t) phase * a.cout32 + co0 + l31) * a.kd16 + 8 * half;
    floatx16c acc;
    #pragma unroll
    for (int r = 0; r < 16; r++) acc[r] = 0.0f;
    auto load_b = [&](int kb) {
        const int kdd = 16 * kb + 8 * half;
        half8 bv;
        #pragma unroll
        for (int e = 0; e < 8; e++) bv[e] = (half_t) 0.0f;
        if (live && kdd < a.kd) {
            const int kk = kdd / a.cin, ci0 = kdd - kk * a.cin;
            const int j = conv_src_row(a.convT, a.K, kk, t, rows);
            if (j >= 0) bv = *reinterpret_cast<const half8 *>(a.xh + (size_t) (row0 + j) * a.cin + ci0);
        }
        return bv;
    };
    // four kd blocks per trip: their eight operand loads are in flight together
    int kb = 0;
    for (; kb + 4 <= nkb; kb += 4) {
        half8 av[4], bv[4];
        #pragma unroll
        for (int i = 0; i < 4; i++) { av[i] = *reinterpret_cast<const half8 *>(wrow + 16 * (kb + i)); bv[i] = load_b(kb + i); }
        #pragma unroll
        for (int i = 0; i < 4; i++) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(av[i], bv[i], acc, 0, 0, 0);
    }
    for (; kb < nkb; kb++) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const half8 *>(wrow + 16 * kb), load_b(kb), acc, 0, 0, 0);
    if (!live) return;
    const size_t orow = a.convT ? (size_t) row * a.nphase + phase : (size_t) row;
    #pragma unroll
    for (int g = 0; g < 4; g++) {
        const int co = co0 + 8 * g + 4 * half;                     // accumulator registers 4 g .. 4 g + 3: channels co .. co + 3 of this lane's row
        #pragma unroll
        for (int e = 0; e < 4; e++) {
            if (co + e >= a.cout) break;
            float v = acc[4 * g + e] + a.bias[co + e];
            const size_t o = orow * a.cout + co + e;
            if (a.add) v = v + a.add[o];
            if (a.y) a.y[o] = v;
            if (a.yh_raw) a.yh_raw[o] = to_half(v);
            if (a.yh_elu) a.yh_elu[o] = to_half(elu_canon(v));
        }
    }
}

// C9: one fmaf chain per output in (ci, k) order, bias last (toy models' narrow convolutions; the cross-check route of C9m)
__global__ __launch_bounds__(256) void conv_tm_chain_kernel(const ConvTmArgs a) {
    const size_t idx = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    const int phase = blockIdx.z;
    if (idx >= (size_t) a.rows_in * a.cout) return;
    const int row = (int) (idx / a.cout), co = (int) (idx % a.cout);
    int row0, rows;
    utt_of_row(a.cb, a.T_single, a.tm_in, row, row0, rows);
    const int t = row - row0;
    float acc = 0.0f;
    if (a.convT) {
        const int s = a.nphase, K = 2 * s;
        for (int ci = 0; ci < a.cin; ci++) {
            const float * wr = a.w32 + ((size_t) ci * a.cout + co) * K;
            if (t > 0) acc = fmaf(wr[phase + s], (float) a.xh[(size_t) (row - 1) * a.cin + ci], acc);
            acc = fmaf(wr[phase], (float) a.xh[(size_t) row * a.cin + ci], acc);
        }
    } else {
        for (int ci = 0; ci < a.cin; ci++) {
            const float * wr = a.w32 + ((size_t) co * a.cin + ci) * a.K;
            for (int k = 0; k < a.K; k++) {
                const int j = conv_src_row(0, a.K, k, t, rows);
                const float xv = j >= 0 ? (float) a.xh[(size_t) (row0 + j) * a.cin + ci] : 0.0f;
                acc = fmaf(wr[k], xv, acc);
            }
        }
    }
    float v = acc + a.bias[co];
    const size_t o = (a.convT ? (size_t) row * a.nphase + phase : (size_t) row) * a.cout + co;
    if (a.add) v = v + a.add[o];
    if (a.y) a.y[o] = v;
    if (a.yh_raw) a.yh_raw[o] = to_half(v);
    if (a.yh_elu) a.yh_elu[o] = to_half(elu_canon(v));
}

void launch_conv_tm(hipStream_t s, const ConvTmArgs & a) {
    if (a.convT && a.K != 2 * a.nphase) kernel_fail("bark-hip: transposed convolution needs kernel == 2 * stride (got %d, %d)", a.K, a.nphase);
    if (a.W && !(crosscheck_mask() & 1024)) {
        hipLaunchKernelGGL(conv_tm_mfma_kernel, dim3((a.rows_in + 127) / 128, a.cout32 / 32, a.nphase), dim3(256), 0, s, a);
        return;
    }
    const size_t n = (size_t) a.rows_in * a.cout;
    hipLaunchKernelGGL(conv_tm_chain_kernel, dim3((unsigned) ((n + 255) / 256), 1, a.nphase), dim3(256), 0, s, a);
}

// one unit (d) of one layer at one step: the four gates in the four 16-lane groups of the wave, C1 dots (lane c of a group = chain c: its
// 8-element chunk of every 128-block, ascending; tree over the 16 lanes), gate non-linearities in double precision rounded once (C9), state
// update by lane 0.  Every operand chunk of the step's dots is requested before the first multiply-add (NBLK = D / 128 is a template
// parameter: with the run-time loop each 128-block was a dependent round trip to L2, eight of them for a unit of the second layer).
template <int NBLK>
__device__ __forceinline__ void lstm_load(half8 (&v)[NBLK], const half_t * row) {
    #pragma unroll
    for (int b = 0; b < NBLK; b++) v[b] = *reinterpret_cast<const half8 *>(row + (b << 7));
}
template <int NBLK>
__device__ __forceinline__ float lstm_dot(const half8 (&w)[NBLK], const half8 (&h)[NBLK]) {
    float acc = 0.0f;
    #pragma unroll
    for (int b = 0; b < NBLK; b++)
        #pragma unroll
        for (int e = 0; e < 8; e++) acc = fmaf((float) w[b][e], (float) h[b][e], acc);
    acc = acc + __shfl_xor(acc, 1, 64); acc = acc + __shfl_xor(acc, 2, 64);
    acc = acc + __shfl_xor(acc, 4, 64); acc = acc + __shfl_xor(acc, 8, 64);
    return acc;
}
template <int NBLK>
__global__ __launch_bounds__(256) void lstm_pair_step_kernel(const LstmPairArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 15, g = lane >> 4;
    constexpr int D = NBLK * 128, nb1 = D / 4;
    const int i = a.t_base ? a.t_base[0] + a.t : a.t;              // launch index: layer 1 at step i, layer 2 at step i - 1
    // utterance blockIdx.z of a batch: T frames, its rows of gi1 / h1 / h2 / out2 start at row0, its cells at D z
    const int z = blockIdx.z;
    const int T = a.cb.T ? a.cb.T[z] : (a.t_base ? a.t_base[1] : a.T);
    const size_t row0 = a.cb.T ? (size_t) a.cb.Tpre[z] : 0;
    const bool second = (int) blockIdx.x >= nb1;
    const int d = ((int) blockIdx.x - (second ? nb1 : 0)) * 4 + wave;
    const int t = second ? i - 1 : i;
    if (t < 0 || t >= T) return;
    const size_t row = (size_t) (g * D + d);
    const half_t * h1 = a.h1 + row0 * D, * h2 = a.h2 + row0 * D;
    float * cs = (second ? a.c2 : a.c1) + (size_t) z * D;
    const float cprev = t ? cs[d] : 0.0f;                          // requested with the operands, not behind the gates
    float gi, gh = 0.0f, bi, bh;
    if (!second) {
        half8 w[NBLK], h[NBLK];
        if (t) { lstm_load<NBLK>(w, a.w_hh1 + row * D + (c << 3)); lstm_load<NBLK>(h, h1 + (size_t) (t - 1) * D + (c << 3)); }
        gi = a.gi1[(row0 + t) * 4 * D + row]; bi = a.b_ih1[row]; bh = a.b_hh1[row];
        if (t) gh = lstm_dot<NBLK>(w, h);
    } else {
        half8 wi[NBLK], hi[NBLK], wh[NBLK], hh[NBLK];
        lstm_load<NBLK>(wi, a.w_ih2 + row * D + (c << 3)); lstm_load<NBLK>(hi, h1 + (size_t) t * D + (c << 3));
        if (t) { lstm_load<NBLK>(wh, a.w_hh2 + row * D + (c << 3)); lstm_load<NBLK>(hh, h2 + (size_t) (t - 1) * D + (c << 3)); }
        bi = a.b_ih2[row]; bh = a.b_hh2[row];
        gi = lstm_dot<NBLK>(wi, hi);                                // W_ih2 . f16(h1_t)
        if (t) gh = lstm_dot<NBLK>(wh, hh);
    }
    const float pre = (gi + bi) + (gh + bh);                   // (gi + b_ih) + (gh + b_hh)
    const float act = g == 2 ? (float) tanh((double) pre) : 1.0f / (1.0f + (float) exp((double) (-pre)));
    const float i_t = __shfl(act, 0, 64), f_t = __shfl(act, 16, 64), g_t = __shfl(act, 32, 64), o_t = __shfl(act, 48, 64);
    if (lane == 0) {
        const float cn = f_t * cprev + i_t * g_t;
        const float hn = o_t * (float) tanh((double) cn);
        cs[d] = cn;
        (second ? a.h2 : a.h1)[(row0 + t) * D + d] = to_half(hn);
        if (second) a.out2[(row0 + t) * D + d] = hn;                // time-major, as every activation of the codec
    }
}
void launch_lstm_pair_step(hipStream_t s, const LstmPairArgs & a) {
    const dim3 grid(2 * (a.D / 4), 1, a.cb.B), block(256);
    switch (a.D >> 7) {
        case 1: hipLaunchKernelGGL((lstm_pair_step_kernel<1>), grid, block, 0, s, a); break;
        case 2: hipLaunchKernelGGL((lstm_pair_step_kernel<2>), grid, block, 0, s, a); break;
        case 4: hipLaunchKernelGGL((lstm_pair_step_kernel<4>), grid, block, 0, s, a); break;
        case 8: hipLaunchKernelGGL((lstm_pair_step_kernel<8>), grid, block, 0, s, a); break;
        default: kernel_fail("bark-hip: the codec's LSTM width must be 128, 256, 512 or 1024 (got %d)", a.D);
    }
}

__global__ void add_int_kernel(int * p, int v) { *p += v; }      // p[0]: step base of the replayed LSTM block
void launch_add_int(hipStream_t s, int * p, int v) { hipLaunchKernelGGL(add_int_kernel, dim3(1), dim3(1), 0, s, p, v); }
__global__ void add_kernel(const float * a, const float * b, size_t n, float * out) {
    for (size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t) gridDim.x * blockDim.x) out[i] = a[i] + b[i];
}
void launch_add(hipStream_t s, const float * a, const float * b, size_t n, float * out) {
    const int blocks = (int) ((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(add_kernel, dim3(blocks), dim3(256), 0, s, a, b, n, out);
}

// ---- EnCodec encoder ------------------------------------------------------------------------------
// EncodecConv1d with a stride (modeling_encodec.py: EncodecConv1d.forward / _pad1d), the 24 kHz model's causal reflect padding: left pad K - stride,
// right pad rows_out * stride - rows (rows_out = ceil(rows / stride)), both by reflection; an input not longer than the larger pad is first extended
// with zeros to that pad + 1 rows, reflected, and the same number of rows is cut off the END of the padded array - every output row reads padded rows
// below that cut, so only the reflection point moves.  Source row of tap kk of output row t; -1: the operand is zero.
__device__ __forceinline__ int conv_down_src_row(int K, int stride, int kk, int t, int rows, int rows_out) {
    const int pl = K - stride, pr = rows_out * stride - rows;
    const int mp = pl > pr ? pl : pr;
    const int Lp = rows <= mp ? mp + 1 : rows;                    // length the reflection sees
    int j = t * stride + kk - pl;
    if (j < 0) j = -j;
    else if (j >= Lp) j = 2 * Lp - 2 - j;
    return (j >= 0 && j < rows) ? j : -1;
}
// valid mode (no padding: the feature encoder of the semantic encoder, C12h): tap kk of output row t is input row t stride + kk, always inside the recording
__device__ __forceinline__ int conv_valid_src_row(int stride, int kk, int t, int rows) {
    const int j = t * stride + kk;
    return j < rows ? j : -1;
}
// exact (erf) GELU, formed in double precision and rounded once - as the LSTM's gate functions are (C9)
__device__ __forceinline__ float gelu_erf_canon(float x) { return (float) (0.5 * (double) x * (1.0 + erf((double) x * 0.70710678118654752440))); }
__device__ __forceinline__ int utt_index_of_row(const CodecBatch & cb, int row) {
    int z = 0;
    while (z + 1 < cb.B && row >= cb.Tpre[z + 1]) z++;
    return z;
}

// C9m, sibling of conv_tm_mfma_kernel: one wave = 32 OUTPUT rows x 32 output channels; the operand rows of a lane are the K input rows of its output row
__global__ __launch_bounds__(256) void conv_down_mfma_kernel(const ConvDownArgs a) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, half = lane >> 5, l31 = lane & 31;
    const int orow = (blockIdx.x * 4 + w) * 32 + l31;             // global output row of this lane's column
    const int co0 = blockIdx.y * 32;
    const bool live = orow < a.rows_out;
    int t = 0, rows = 0, rows_out = 0, in0 = 0;
    if (live) {
        const int z = utt_index_of_row(a.cb_out, orow);
        t = orow - a.cb_out.Tpre[z]; rows_out = a.cb_out.T[z]; rows = a.cb_in.T[z]; in0 = a.cb_in.Tpre[z];
    }
    const int nkb = a.kd16 >> 4;
    const half_t * wrow = a.W + ((size_t) co0 + l31) * a.kd16 + 8 * half;
    floatx16c acc;
    #pragma unroll
    for (int r = 0; r < 16; r++) acc[r] = 0.0f;
    auto load_b = [&](int kb) {
        const int kdd = 16 * kb + 8 * half;
        half8 bv;
        #pragma unroll
        for (int e = 0; e < 8; e++) bv[e] = (half_t) 0.0f;
        if (live && kdd < a.kd) {
            const int kk = kdd / a.cin, ci0 = kdd - kk * a.cin;
            const int j = a.valid ? conv_valid_src_row(a.stride, kk, t, rows) : conv_down_src_row(a.K, a.stride, kk, t, rows, rows_out);
            if (j >= 0) bv = *reinterpret_cast<const half8 *>(a.xh + (size_t) (in0 + j) * a.cin + ci0);
        }
        return bv;
    };
    int kb = 0;
    for (; kb + 4 <= nkb; kb += 4) {
        half8 av[4], bv[4];
        #pragma unroll
        for (int i = 0; i < 4; i++) { av[i] = *reinterpret_cast<const half8 *>(wrow + 16 * (kb + i)); bv[i] = load_b(kb + i); }
        #pragma unroll
        for (int i = 0; i < 4; i++) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(av[i], bv[i], acc, 0, 0, 0);
    }
    for (; kb < nkb; kb++) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const half8 *>(wrow + 16 * kb), load_b(kb), acc, 0, 0, 0);
    if (!live) return;
    #pragma unroll
    for (int g = 0; g < 4; g++) {
        const int co = co0 + 8 * g + 4 * half;
        #pragma unroll
        for (int e = 0; e < 4; e++) {
            if (co + e >= a.cout) break;
            float v = acc[4 * g + e];
            if (a.bias) v = v + a.bias[co + e];
            const size_t o = (size_t) orow * a.cout + co + e;
            if (a.y) a.y[o] = v;
            if (a.yh_raw) a.yh_raw[o] = to_half(v);
            if (a.yh_elu) a.yh_elu[o] = to_half(elu_canon(v));
            if (a.y_gelu || a.yh_gelu) {
                const float ge = gelu_erf_canon(v);
                if (a.y_gelu) a.y_gelu[o] = ge;
                if (a.yh_gelu) a.yh_gelu[o] = to_half(ge);
            }
        }
    }
}

// C9: one fmaf chain per output in (ci, k) order, bias last
__global__ __launch_bounds__(256) void conv_down_chain_kernel(const ConvDownArgs a) {
    const size_t idx = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t) a.rows_out * a.cout) return;
    const int orow = (int) (idx / a.cout), co = (int) (idx % a.cout);
    const int z = utt_index_of_row(a.cb_out, orow);
    const int t = orow - a.cb_out.Tpre[z], rows_out = a.cb_out.T[z], rows = a.cb_in.T[z], in0 = a.cb_in.Tpre[z];
    float acc = 0.0f;
    for (int ci = 0; ci < a.cin; ci++) {
        const float * wr = a.w32 + ((size_t) co * a.cin + ci) * a.K;
        for (int k = 0; k < a.K; k++) {
            const int j = a.valid ? conv_valid_src_row(a.stride, k, t, rows) : conv_down_src_row(a.K, a.stride, k, t, rows, rows_out);
            const float xv = j >= 0 ? (float) a.xh[(size_t) (in0 + j) * a.cin + ci] : 0.0f;
            acc = fmaf(wr[k], xv, acc);
        }
    }
    float v = acc;
    if (a.bias) v = v + a.bias[co];
    if (a.y) a.y[idx] = v;
    if (a.yh_raw) a.yh_raw[idx] = to_half(v);
    if (a.yh_elu) a.yh_elu[idx] = to_half(elu_canon(v));
    if (a.y_gelu || a.yh_gelu) {
        const float ge = gelu_erf_canon(v);
        if (a.y_gelu) a.y_gelu[idx] = ge;
        if (a.yh_gelu) a.yh_gelu[idx] = to_half(ge);
    }
}

void launch_conv_down(hipStream_t s, const ConvDownArgs & a) {
    if (a.stride < 1 || a.K < a.stride || !a.cb_in.T || !a.cb_out.T) kernel_fail("bark-hip: strided convolution needs kernel >= stride >= 1 and both stages' row tables (got %d, %d)", a.K, a.stride);
    if (a.W && !(crosscheck_mask() & 1024)) {
        hipLaunchKernelGGL(conv_down_mfma_kernel, dim3((a.rows_out + 127) / 128, a.cout32 / 32), dim3(256), 0, s, a);
        return;
    }
    const size_t n = (size_t) a.rows_out * a.cout;
    hipLaunchKernelGGL(conv_down_chain_kernel, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, s, a);
}

// C11q: kRvqFrames frames per workgroup, their residuals in LDS; work-item i scores the codebook rows i, i + 256, .. against all of them (one read of
// a row serves every frame), each distance one chain over d ascending: t = r_d - e_jd; p = t * t; acc = acc + p (-ffp-contract=off: nothing fused).
// The pick is the smallest distance, ties to the lowest row: in the work-item by scanning its rows in ascending order, across work-items by comparing (d, j).
// A frame in which no distance compared below +inf (a non-finite latent, or squares that overflow) has no pick: its code is -1 at this and every later
// stage, its residual is left alone, and the host turns the -1 into an error (engine_codec.hip) - never a code.
constexpr int kRvqFrames = 4, kRvqMaxDim = 1024;
__global__ __launch_bounds__(256) void rvq_encode_kernel(const float * codebooks, int n_bins, int Hd, const float * z, int n_q, int rows_total, int32_t * codes, const CodecBatch cb) {
    __shared__ float r[kRvqFrames * kRvqMaxDim];
    __shared__ float wd[4 * kRvqFrames];
    __shared__ int wj[4 * kRvqFrames];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int f0 = blockIdx.x * kRvqFrames;
    const int nf = min(kRvqFrames, rows_total - f0);
    for (int i = tid; i < kRvqFrames * Hd; i += 256) {
        const int f = i / Hd, d = i - f * Hd;
        r[f * kRvqMaxDim + d] = f < nf ? z[(size_t) (f0 + f) * Hd + d] : 0.0f;
    }
    __syncthreads();
    for (int q = 0; q < n_q; q++) {
        const float * E = codebooks + (size_t) q * n_bins * Hd;
        float best[kRvqFrames]; int bj[kRvqFrames];
        #pragma unroll
        for (int f = 0; f < kRvqFrames; f++) { best[f] = INFINITY; bj[f] = 0x7fffffff; }
        for (int j = tid; j < n_bins; j += 256) {
            const float * e = E + (size_t) j * Hd;
            float acc[kRvqFrames];
            #pragma unroll
            for (int f = 0; f < kRvqFrames; f++) acc[f] = 0.0f;
            int d = 0;
            if (!(Hd & 3)) {
                for (; d < Hd; d += 4) {
                    const float4 ev = *reinterpret_cast<const float4 *>(e + d);
                    #pragma unroll
                    for (int f = 0; f < kRvqFrames; f++) {
                        const float * rf = r + f * kRvqMaxDim + d;
                        float t = rf[0] - ev.x; float p = t * t; acc[f] = acc[f] + p;
                        t = rf[1] - ev.y; p = t * t; acc[f] = acc[f] + p;
                        t = rf[2] - ev.z; p = t * t; acc[f] = acc[f] + p;
                        t = rf[3] - ev.w; p = t * t; acc[f] = acc[f] + p;
                    }
                }
            }
            for (; d < Hd; d++) {
                const float ev = e[d];
                #pragma unroll
                for (int f = 0; f < kRvqFrames; f++) { const float t = r[f * kRvqMaxDim + d] - ev; const float p = t * t; acc[f] = acc[f] + p; }
            }
            #pragma unroll
            for (int f = 0; f < kRvqFrames; f++) if (acc[f] < best[f]) { best[f] = acc[f]; bj[f] = j; }
        }
        #pragma unroll
        for (int f = 0; f < kRvqFrames; f++) {
            for (int m = 1; m < 64; m <<= 1) {
                const float od = __shfl_xor(best[f], m, 64); const int oj = __shfl_xor(bj[f], m, 64);
                if (od < best[f] || (od == best[f] && oj < bj[f])) { best[f] = od; bj[f] = oj; }
            }
            if (lane == 0) { wd[wave * kRvqFrames + f] = best[f]; wj[wave * kRvqFrames + f] = bj[f]; }
        }
        __syncthreads();
        int pick[kRvqFrames];
        #pragma unroll
        for (int f = 0; f < kRvqFrames; f++) {
            float bd = wd[f]; int b = wj[f];
            for (int w = 1; w < 4; w++) {
                const float od = wd[w * kRvqFrames + f]; const int oj = wj[w * kRvqFrames + f];
                if (od < bd || (od == bd && oj < b)) { bd = od; b = oj; }
            }
            pick[f] = b < n_bins ? b : -1;
        }
        #pragma unroll
        for (int f = 0; f < kRvqFrames; f++) {
            if (pick[f] >= 0) {
                const float * e = E + (size_t) pick[f] * Hd;
                for (int d = tid; d < Hd; d += 256) r[f * kRvqMaxDim + d] = r[f * kRvqMaxDim + d] - e[d];
            }
            if (tid == f && f < nf) {
                int row0, rows;
                utt_of_row(cb, 0, 1, f0 + f, row0, rows);
                codes[(size_t) n_q * row0 + (size_t) q * rows + (f0 + f - row0)] = pick[f];
            }
        }
        __syncthreads();
    }
}
void launch_rvq_encode(hipStream_t s, const float * codebooks, int n_bins, int Hd, const float * z, int n_q, int rows_total, int32_t * codes, const CodecBatch & cb) {
    if (Hd < 1 || Hd > kRvqMaxDim || !cb.T) kernel_fail("bark-hip: the RVQ encoder takes latents of 1..%d dimensions (got %d)", kRvqMaxDim, Hd);
    hipLaunchKernelGGL(rvq_encode_kernel, dim3((rows_total + kRvqFrames - 1) / kRvqFrames), dim3(256), 0, s, codebooks, n_bins, Hd, z, n_q, rows_total, codes, cb);
}

// ---- semantic encoder (HuBERT feature encoder and positional convolution; rule C12h) --------------------------------
// Convolution 0 (one input channel, K taps, stride s, no bias) with its per-channel norm over time.  T0 reaches 65 615 rows: the f32 result is never
// stored, each output is one fmaf chain over k ascending and is formed twice.  Pass 1: work-item = channel, workgroup = kHubChunk consecutive rows; sum and
// sum of squares of its rows in double precision, rows ascending.  Pass 2: the chunks' partial sums added in ascending order (a fixed tree: chain inside a
// chunk, chain over chunks), mean = S / T0, var = SS / T0 - mean^2 (biased), both in double; rstd = 1 / sqrt(var + 1e-5) rounded to f32 once.  Pass 3:
// ((y - mean) rstd) g + b in f32, erf GELU, f16 image (and the f32 value for the parity tap).
constexpr int kHubChunk = 1024, kHubMaxK0 = 16;
__device__ __forceinline__ float hub_conv0_dot(const half_t * w, const half_t * x, int K) {
    float acc = 0.0f;
    for (int k = 0; k < K; k++) acc = fmaf((float) w[k], (float) x[k], acc);
    return acc;
}
__global__ __launch_bounds__(128) void hub_conv0_stats_kernel(const HubConv0Args a) {
    const int c = blockIdx.y * 128 + threadIdx.x;
    if (c >= a.C) return;
    half_t w[kHubMaxK0];
    for (int k = 0; k < a.K; k++) w[k] = a.w[(size_t) c * a.K + k];
    const int t0 = blockIdx.x * kHubChunk, t1 = min(a.T0, t0 + kHubChunk);
    double s = 0.0, ss = 0.0;
    for (int t = t0; t < t1; t++) {
        const double y = (double) hub_conv0_dot(w, a.xh + (size_t) t * a.stride, a.K);
        s = s + y; ss = ss + y * y;
    }
    double * p = a.part + ((size_t) blockIdx.x * a.C + c) * 2;
    p[0] = s; p[1] = ss;
}
__global__ __launch_bounds__(128) void hub_conv0_final_kernel(const HubConv0Args a) {
    const int c = blockIdx.x * 128 + threadIdx.x;
    if (c >= a.C) return;
    const int nchunk = (a.T0 + kHubChunk - 1) / kHubChunk;
    double s = 0.0, ss = 0.0;
    for (int i = 0; i < nchunk; i++) { s = s + a.part[((size_t) i * a.C + c) * 2]; ss = ss + a.part[((size_t) i * a.C + c) * 2 + 1]; }
    const double mean = s / (double) a.T0;
    double var = ss / (double) a.T0 - mean * mean;
    if (var < 0.0) var = 0.0;
    a.stats[2 * c] = (float) mean;
    a.stats[2 * c + 1] = (float) (1.0 / sqrt(var + 1e-5));
}
__global__ __launch_bounds__(256) void hub_conv0_emit_kernel(const HubConv0Args a) {
    const size_t idx = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t) a.T0 * a.C) return;
    const int t = (int) (idx / a.C), c = (int) (idx % a.C);
    const float y = hub_conv0_dot(a.w + (size_t) c * a.K, a.xh + (size_t) t * a.stride, a.K);
    float v = (y - a.stats[2 * c]) * a.stats[2 * c + 1];
    v = v * a.g[c];
    v = v + a.b[c];
    const float ge = gelu_erf_canon(v);
    a.yh[idx] = to_half(ge);
    if (a.y) a.y[idx] = ge;
}
void launch_hub_conv0(hipStream_t s, const HubConv0Args & a) {
    if (a.K < 1 || a.K > kHubMaxK0 || a.stride < 1 || a.T0 < 1 || (size_t) (a.T0 - 1) * a.stride + a.K > (size_t) a.n)
        kernel_fail("bark-hip: the first feature convolution takes 1..%d taps and rows inside the recording (got K %d, stride %d, T0 %d, n %d)", kHubMaxK0, a.K, a.stride, a.T0, a.n);
    const int nchunk = (a.T0 + kHubChunk - 1) / kHubChunk, cg = (a.C + 127) / 128;
    hipLaunchKernelGGL(hub_conv0_stats_kernel, dim3(nchunk, cg), dim3(128), 0, s, a);
    hipLaunchKernelGGL(hub_conv0_final_kernel, dim3(cg), dim3(128), 0, s, a);
    const size_t n = (size_t) a.T0 * a.C;
    hipLaunchKernelGGL(hub_conv0_emit_kernel, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, s, a);
}
int hub_conv0_chunks(int T0) { return (T0 + kHubChunk - 1) / kHubChunk; }

// Grouped positional convolution (Conv1d(H, H, Kp, padding Kp / 2, groups G), for even Kp without its last output frame) on the f16 matrix cores, order
// C9m per group: output row t, channel g Hg + co = bias + sum over kd = k Hg + ci of w[g Hg + co][ci][k] x[t + k - Kp / 2][g Hg + ci] (rows outside the
// recording are zero).  The operand run of tap k is the Hg-element slice of ONE time row, so a lane's 8 consecutive kd never leave a row (Hg % 8 == 0).
// One wave = 32 rows x 32 channels of one group (the image of a group is padded to co32 rows); epilogue: erf GELU in f32 - the value joins an f32 sum.
__global__ __launch_bounds__(256) void pos_conv_mfma_kernel(const PosConvArgs a) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, half = lane >> 5, l31 = lane & 31;
    const int t = (blockIdx.x * 4 + w) * 32 + l31;
    const int ct = a.co32 >> 5, grp = blockIdx.y / ct, ctile = blockIdx.y - grp * ct;
    const int Hg = a.H / a.G, pad = a.Kp >> 1;
    const bool live = t < a.T;
    const int nkb = a.kd16 >> 4;
    const half_t * wrow = a.W + ((size_t) grp * a.co32 + ctile * 32 + l31) * a.kd16 + 8 * half;
    floatx16c acc;
    #pragma unroll
    for (int r = 0; r < 16; r++) acc[r] = 0.0f;
    auto load_b = [&](int kb) {
        const int kdd = 16 * kb + 8 * half;
        half8 bv;
        #pragma unroll
        for (int e = 0; e < 8; e++) bv[e] = (half_t) 0.0f;
        if (live && kdd < a.kd) {
            const int kk = kdd / Hg, ci0 = kdd - kk * Hg;
            const int j = t + kk - pad;
            if (j >= 0 && j < a.T) bv = *reinterpret_cast<const half8 *>(a.xh + (size_t) j * a.H + grp * Hg + ci0);
        }
        return bv;
    };
    int kb = 0;
    for (; kb + 4 <= nkb; kb += 4) {
        half8 av[4], bv[4];
        #pragma unroll
        for (int i = 0; i < 4; i++) { av[i] = *reinterpret_cast<const half8 *>(wrow + 16 * (kb + i)); bv[i] = load_b(kb + i); }
        #pragma unroll
        for (int i = 0; i < 4; i++) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(av[i], bv[i], acc, 0, 0, 0);
    }
    for (; kb < nkb; kb++) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const half8 *>(wrow + 16 * kb), load_b(kb), acc, 0, 0, 0);
    if (!live) return;
    #pragma unroll
    for (int g = 0; g < 4; g++) {
        const int co = ctile * 32 + 8 * g + 4 * half;
        #pragma unroll
        for (int e = 0; e < 4; e++) {
            if (co + e >= Hg) break;
            const int ch = grp * Hg + co + e;
            const float v = acc[4 * g + e] + a.bias[ch];
            a.y[(size_t) t * a.H + ch] = gelu_erf_canon(v);
        }
    }
}
void launch_pos_conv(hipStream_t s, const PosConvArgs & a) {
    if (a.G < 1 || a.H % a.G || ((a.H / a.G) & 7) || (a.co32 & 31) || a.co32 < a.H / a.G || a.kd != a.Kp * (a.H / a.G) || (a.kd16 & 15) || a.kd16 < a.kd || a.T < 1)
        kernel_fail("bark-hip: the positional convolution needs groups of a multiple of 8 channels and a padded kernel image (got H %d, G %d, Kp %d)", a.H, a.G, a.Kp);
    hipLaunchKernelGGL(pos_conv_mfma_kernel, dim3((a.T + 127) / 128, a.G * (a.co32 / 32)), dim3(256), 0, s, a);
}

// ---- 24 kHz -> 16 kHz resampler (rule C13r) ----------------------------------------------------------------------------------
// Output m sits at input time t = 1.5 m: base = floor(t), phase = m % 2, y[m] = the fmaf chain acc = fmaf(x[base + j], h[phase][j + 10], acc) over j = -10 .. 11
// ascending from acc = +0, zero taps included, samples outside the recording +0, no renormalisation.  The taps are the f32 roundings of the double-precision
// values of c sinc(c u) cos^2(pi u / (2 W)) (|u| < W, else 0) at u = phase / 2 - j, c = 0.99 * 2 / 3, W = 6 / c (bark.cpp_amd/voice.py resample_24k_to_16k): a
// committed table, never computed at load time - a libm's sin / cos may differ from numpy's in the last place.
// One workgroup = 512 consecutive outputs = 768 input samples + 10 in front + 12 behind, staged once in LDS as 198 16-byte loads from the 16-byte boundary
// 12 samples in front of the tile; work-item t forms the pair m = 2 k, 2 k + 1 (k = 256 blockIdx.x + t) from the 23 samples x[3 k - 10 .. 3 k + 12] (LDS
// stride 3 between lanes: no bank conflict) and writes it as one 8-byte store.  The taps travel as a kernel argument (scalar registers).
constexpr int kRsTile = 512, kRsIn = 768, kRsLead = 12, kRsWin4 = (kRsIn + 2 * kRsLead) / 4;
struct ResampleTaps { float h[44]; };
static const float kResampleTaps[44] = {
    // phase 0 (even m), j = -10 .. 11
    0.000000000e+00f, -1.635075932e-06f, -1.076447428e-03f, 5.282599479e-03f, -1.722944784e-03f, -2.172333933e-02f, 4.274801165e-02f, -5.026828963e-03f,
    -1.189598665e-01f, 2.706918120e-01f, 6.600000262e-01f, 2.706918120e-01f, -1.189598665e-01f, -5.026828963e-03f, 4.274801165e-02f, -2.172333933e-02f,
    -1.722944784e-03f, 5.282599479e-03f, -1.076447428e-03f, -1.635075932e-06f, 0.000000000e+00f, -0.000000000e+00f,
    // phase 1 (odd m), j = -10 .. 11
    0.000000000e+00f, 0.000000000e+00f, -3.660349757e-04f, 4.891819553e-04f, 7.250521332e-03f, -1.795493253e-02f, 3.380680922e-03f, 5.090378597e-02f,
    -9.356202930e-02f, 6.227747072e-03f, 5.438855886e-01f, 5.438855886e-01f, 6.227747072e-03f, -9.356202930e-02f, 5.090378597e-02f, 3.380680922e-03f,
    -1.795493253e-02f, 7.250521332e-03f, 4.891819553e-04f, -3.660349757e-04f, 0.000000000e+00f, 0.000000000e+00f,
};
const float * resample_taps() { return kResampleTaps; }

__global__ __launch_bounds__(256) void resample_24k_16k_kernel(const float * x, int n, float * y, int n_out, int vec, const ResampleTaps taps) {
    __shared__ float4 win4[kRsWin4];
    const int t = (int) threadIdx.x;
    if (t < kRsWin4) {
        const int g = (int) blockIdx.x * kRsIn - kRsLead + 4 * t;       // first of this work-item's four samples; a multiple of 4
        float4 v;
        if (vec && g >= 0 && g + 3 < n) v = *reinterpret_cast<const float4 *>(x + g);
        else {
            v.x = (g >= 0 && g < n) ? x[g] : 0.0f;
            v.y = (g + 1 >= 0 && g + 1 < n) ? x[g + 1] : 0.0f;
            v.z = (g + 2 >= 0 && g + 2 < n) ? x[g + 2] : 0.0f;
            v.w = (g + 3 >= 0 && g + 3 < n) ? x[g + 3] : 0.0f;
        }
        win4[t] = v;
    }
    __syncthreads();
    const int m = (int) blockIdx.x * kRsTile + 2 * t;
    if (m >= n_out) return;
    const float * w = reinterpret_cast<const float *>(win4) + 3 * t + (kRsLead - 10);      // x[3 k - 10]
    float xv[23];
    #pragma unroll
    for (int i = 0; i < 23; i++) xv[i] = w[i];
    float a0 = 0.0f, a1 = 0.0f;
    #pragma unroll
    for (int i = 0; i < 22; i++) {
        a0 = fmaf(xv[i], taps.h[i], a0);                 // base 3 k:     x[3 k - 10 + i]
        a1 = fmaf(xv[i + 1], taps.h[22 + i], a1);        // base 3 k + 1: x[3 k - 9 + i]
    }
    if (m + 1 >= n_out) y[m] = a0;
    else if (vec) *reinterpret_cast<float2 *>(y + m) = make_float2(a0, a1);
    else { y[m] = a0; y[m + 1] = a1; }
}
void launch_resample_24k_16k(hipStream_t s, const float * x, int n, float * y, int n_out) {
    if (!x || !y || n < 1 || n > kResampleMaxSamples || n_out != (2 * n + 2) / 3)
        kernel_fail("bark-hip: the resampler takes 1 .. %d samples and writes (2 n + 2) / 3 (got n %d, n_out %d)", kResampleMaxSamples, n, n_out);
    ResampleTaps taps;
    for (int i = 0; i < 44; i++) taps.h[i] = kResampleTaps[i];
    const int vec = (((size_t) x & 15) == 0 && ((size_t) y & 7) == 0) ? 1 : 0;
    hipLaunchKernelGGL(resample_24k_16k_kernel, dim3((n_out + kRsTile - 1) / kRsTile), dim3(256), 0, s, x, n, y, n_out, vec, taps);
}

// ---- rational resampler and the sample formats (rule C14r) ----------------------------------------------------------------------
// The general form of the kernel above: any L / M, up to 160 phases of up to 40 taps - too large for a kernel argument, so the table lives in a device
// buffer (uploaded once per pair and context) and every workgroup copies it into LDS, rows 2 half + 1 floats apart (consecutive outputs read consecutive
// phase rows: an odd row distance spreads them over the banks).  One workgroup = one tile of 1024 consecutive outputs of ONE segment (the tile table of
// `seg` says which): it stages the input window x[base(m0) - half + 1 .. base(m0 + cnt - 1) + half] once, as 16-byte loads from the 16-byte boundary at or
// below the window's first sample - a segment starts anywhere in x, so the boundary is found from in_off + the window's start - and sample by sample, zero
// outside the segment, where a quad crosses the segment's ends or x itself is not 16-byte aligned.  Work-item t forms outputs m0 + t + 256 i: neighbours
// read LDS M / L <= 3 floats apart and store side by side.  Index arithmetic: m M is formed in 64 bits once per tile (m0 M = base0 L + ph0); inside the tile
// (ph0 + d M) < 2^18 gives base and phase in 32 bits.
__device__ __forceinline__ int sample_s16(float y) {
    const float r = rintf(y * 32768.0f);                                 // ties to even; the product is exact (a power of two) or infinite
    return (int) fminf(fmaxf(r, -32768.0f), 32767.0f);                   // saturates; a NaN (a chain that overflowed both ways) goes to -32768
}
__device__ __forceinline__ unsigned sample_mulaw(int s) {
    const unsigned sign = s < 0 ? 0x80u : 0u;
    const int mag = min(s < 0 ? -s : s, 32635) + 132;                    // 132 .. 32767
    const int e = (mag >= 256) + (mag >= 512) + (mag >= 1024) + (mag >= 2048) + (mag >= 4096) + (mag >= 8192) + (mag >= 16384);      // floor(log2 mag) - 7
    const unsigned man = ((unsigned) mag >> (e + 3)) & 15u;
    return ~(sign | ((unsigned) e << 4) | man) & 0xFFu;
}
__device__ __forceinline__ void store_sample(void * y, size_t i, float v, int fmt) {
    if (fmt == 0) static_cast<float *>(y)[i] = v;
    else if (fmt == 1) static_cast<int16_t *>(y)[i] = (int16_t) sample_s16(v);
    else static_cast<uint8_t *>(y)[i] = (uint8_t) sample_mulaw(sample_s16(v));
}

__global__ __launch_bounds__(256) void resample_pair_kernel(const ResamplePairArgs a, int vec) {
    __shared__ float4 win4[kResampleWinFloats / 4];
    __shared__ float tab[kResampleTabFloats];
    constexpr int S = kResampleMaxSegments + 1;
    const int t = (int) threadIdx.x, tile = (int) blockIdx.x;
    const int * tile_off = a.seg + 4 * S;
    int s = 0;
    for (int hi = a.B; hi - s > 1;) { const int mid = (s + hi) >> 1; if (tile_off[mid] <= tile) s = mid; else hi = mid; }      // tile_off[s] <= tile < tile_off[s + 1]
    const int n = a.seg[s], in_off = a.seg[S + s], n_out = a.seg[2 * S + s], out_off = a.seg[3 * S + s];
    const int nt = 2 * a.half, ld = nt + 1;
    for (int i = t; i < a.L * nt; i += 256) { const int p = i / nt; tab[p * ld + (i - p * nt)] = a.taps[i]; }
    const int m0 = (tile - tile_off[s]) * kResampleTile;
    const int cnt = min(kResampleTile, n_out - m0);
    const long long t0 = (long long) m0 * a.M;
    const int base0 = (int) (t0 / a.L), ph0 = (int) (t0 - (long long) base0 * a.L);
    const int last = base0 + (ph0 + (cnt - 1) * a.M) / a.L;              // base of the tile's last output
    const int w0 = base0 - a.half + 1;                                   // the first sample the tile reads, counted from the segment's start (may be < 0)
    const int mis = (in_off + w0) & 3;                                   // samples between the 16-byte boundary and w0 (two's complement: also for a negative sum)
    const int nq = (last + a.half - (w0 - mis)) / 4 + 1;                 // quads that cover w0 - mis .. last + half
    const float * xs0 = a.x + in_off;
    for (int q = t; q < nq; q += 256) {
        const int r = w0 - mis + 4 * q;
        float4 v;
        if (vec && r >= 0 && r + 3 < n) v = *reinterpret_cast<const float4 *>(xs0 + r);
        else {
            v.x = (r >= 0 && r < n) ? xs0[r] : 0.0f;
            v.y = (r + 1 >= 0 && r + 1 < n) ? xs0[r + 1] : 0.0f;
            v.z = (r + 2 >= 0 && r + 2 < n) ? xs0[r + 2] : 0.0f;
            v.w = (r + 3 >= 0 && r + 3 < n) ? xs0[r + 3] : 0.0f;
        }
        win4[q] = v;
    }
    __syncthreads();
    const float * w = reinterpret_cast<const float *>(win4) + mis;       // w[b] = x[base0 + b - half + 1]
    for (int d = t; d < cnt; d += 256) {
        const int k = ph0 + d * a.M;
        const int b = k / a.L;
        const float * xv = w + b, * h = tab + (k - b * a.L) * ld;
        float acc = 0.0f;
        for (int i = 0; i < nt; i++) acc = fmaf(xv[i], h[i], acc);
        store_sample(a.y, (size_t) out_off + (size_t) (m0 + d), acc, a.fmt);
    }
}
void launch_resample_pair(hipStream_t s, const ResamplePairArgs & a, int n_tiles) {
    if (!a.x || !a.y || !a.taps || !a.seg || a.B < 1 || a.B > kResampleMaxSegments || a.L < 1 || a.M < 1 || a.half < 1 || a.fmt < 0 || a.fmt > 2 || n_tiles < a.B ||
        a.L * (2 * a.half + 1) > kResampleTabFloats || (long long) (kResampleTile - 1) * a.M / a.L + 2 * a.half + 8 > kResampleWinFloats)
        kernel_fail("bark-hip: the rational resampler takes 1 .. %d segments and a table that fits its LDS copy (got B %d, L %d, M %d, half %d)", kResampleMaxSegments, a.B, a.L, a.M, a.half);
    const int vec = ((size_t) a.x & 15) == 0 ? 1 : 0;
    hipLaunchKernelGGL(resample_pair_kernel, dim3(n_tiles), dim3(256), 0, s, a, vec);
}

__global__ __launch_bounds__(256) void sample_format_kernel(const float * x, void * y, size_t n, int fmt) {
    const size_t i = (size_t) blockIdx.x * 256 + threadIdx.x;
    if (i < n) store_sample(y, i, x[i], fmt);
}
void launch_sample_format(hipStream_t s, const float * x, void * y, size_t n, int fmt) {
    if (!x || !y || n < 1 || fmt < 1 || fmt > 2) kernel_fail("bark-hip: the sample format kernel takes fmt 1 (s16) or 2 (mu-law) and at least one sample");
    hipLaunchKernelGGL(sample_format_kernel, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, s, x, y, n, fmt);
}

// ---- long-form join (rule C15j) ---------------------------------------------------------------------------------------------------
// Activity: one wave per frame of 240 samples (four frames a workgroup), all segments in one launch.  The peak is a maximum of |x| - exact in any order -
// folded over the wave by xor shuffles; lane 0 of an active frame moves the segment's two table entries by atomicMax, and only when the entry it reads does
// not already cover the frame (the entries move one way, so a stale read costs an atomic, never a result).
__global__ __launch_bounds__(256) void segment_activity_kernel(const JoinActivityArgs a, int n_frames) {
    constexpr int S = kResampleMaxSegments + 1;
    const int lane = (int) threadIdx.x & 63;
    const int f = (int) blockIdx.x * 4 + ((int) threadIdx.x >> 6);       // wave-uniform
    const bool valid = f < n_frames;
    const int * frame_off = a.seg + 2 * S;
    int s = 0, j = 0;
    float peak = 0.0f;
    if (valid) {
        for (int hi = a.B; hi - s > 1;) { const int mid = (s + hi) >> 1; if (frame_off[mid] <= f) s = mid; else hi = mid; }      // frame_off[s] <= f < frame_off[s + 1]
        j = f - frame_off[s];
        const int n = a.seg[s];
        const float * x = a.x + a.seg[S + s];
        const int end = min(kJoinFrame * (j + 1), n);
        for (int i = kJoinFrame * j + lane; i < end; i += 64) peak = fmaxf(peak, fabsf(x[i]));
    }
    for (int off = 32; off > 0; off >>= 1) peak = fmaxf(peak, __shfl_xor(peak, off, 64));
    if (valid && lane == 0 && peak >= a.thr) {
        int * first = a.act + 2 * s, * last = first + 1;
        if (-j > *(volatile int *) first) atomicMax(first, -j);
        if (j > *(volatile int *) last) atomicMax(last, j);
    }
}
void launch_segment_activity(hipStream_t s, const JoinActivityArgs & a, int n_frames) {
    if (!a.x || !a.seg || !a.act || a.B < 1 || a.B > kResampleMaxSegments || n_frames < a.B || !(a.thr >= 0.0f))
        kernel_fail("bark-hip: the activity kernel takes 1 .. %d segments, at least a frame each, and a threshold >= 0 (got B %d, frames %d)", kResampleMaxSegments, a.B, n_frames);
    hipLaunchKernelGGL(segment_activity_kernel, dim3((unsigned) ((n_frames + 3) / 4)), dim3(256), 0, s, a, n_frames);
}

// Join: resample_pair_kernel with another staging loop.  One workgroup = one tile of 1024 consecutive outputs of the joined signal J, which exists only
// as the position table (copied into LDS): while it stages the tile's window, work-item i resolves J's index w0 + i to (range, offset) by binary search
// over the ranges' first samples, reads the sample from its segment, applies the fade weight and writes +0 between the ranges and outside J - once per
// staged sample, not once per tap.  Consecutive work-items write consecutive LDS words; the compute loop is resample_pair_kernel's (tap rows an odd
// distance apart).  m M is formed in 64 bits once per tile (m < 2^26, M <= 160).  The identity has no table: the staged sample itself is stored.
__global__ __launch_bounds__(256) void join_resample_kernel(const JoinResampleArgs a) {
    __shared__ float win[kResampleWinFloats];
    __shared__ float tab[kResampleTabFloats];
    __shared__ int pos[3 * kResampleMaxSegments];
    const int t = (int) threadIdx.x, tile = (int) blockIdx.x;
    const int nt = 2 * a.half, ld = nt + 1;
    if (a.taps) for (int i = t; i < a.L * nt; i += 256) { const int p = i / nt; tab[p * ld + (i - p * nt)] = a.taps[i]; }
    if (t < 3 * kResampleMaxSegments) pos[t] = a.pos[t];
    const int * start = pos, * len = pos + kResampleMaxSegments, * src = pos + 2 * kResampleMaxSegments;
    const int m0 = tile * kResampleTile;
    const int cnt = min(kResampleTile, a.n_out - m0);
    const long long t0 = (long long) m0 * a.M;
    const int base0 = (int) (t0 / a.L), ph0 = (int) (t0 - (long long) base0 * a.L);
    const int last = base0 + (ph0 + (cnt - 1) * a.M) / a.L;              // base of the tile's last output
    const int w0 = base0 - a.half + 1;                                   // the first sample of J the tile reads (may be < 0)
    const int nwin = last + a.half - w0 + 1;
    __syncthreads();
    for (int i = t; i < nwin; i += 256) {
        const int v = w0 + i;
        float x = 0.0f;
        if (v >= 0 && v < a.N) {
            int r = 0;
            for (int hi = a.R; hi - r > 1;) { const int mid = (r + hi) >> 1; if (start[mid] <= v) r = mid; else hi = mid; }      // start[r] <= v (start[0] == 0)
            const int off = v - start[r], K = len[r];
            if (off < K) {
                x = a.x[(size_t) src[r] + (size_t) off];
                const int d = min(off, K - 1 - off);
                if (d < a.F) x = x * a.fade[d];
            }
        }
        win[i] = x;                                                      // win[b] = J[base0 + b - half + 1]
    }
    __syncthreads();
    for (int d = t; d < cnt; d += 256) {
        const int k = ph0 + d * a.M;
        const int b = k / a.L;
        float acc = 0.0f;
        if (a.taps) {
            const float * xv = win + b, * h = tab + (k - b * a.L) * ld;
            for (int i = 0; i < nt; i++) acc = fmaf(xv[i], h[i], acc);
        } else acc = win[b];
        store_sample(a.y, (size_t) (m0 + d), acc, a.fmt);
    }
}
void launch_join_resample(hipStream_t s, const JoinResampleArgs & a) {
    const bool identity = !a.taps;
    if (!a.x || !a.y || !a.pos || a.R < 1 || a.R > kResampleMaxSegments || a.F < 0 || a.F > kJoinMaxFade || (a.F && !a.fade) || a.N < 1 || a.N > kJoinMaxSamples ||
        a.L < 1 || a.M < 1 || a.half < 1 || a.fmt < 0 || a.fmt > 2 || (identity && (a.L != 1 || a.M != 1 || a.half != 1)) ||
        (long long) a.n_out != ((long long) a.N * a.L + a.M - 1) / a.M || a.L * (2 * a.half + 1) > kResampleTabFloats ||
        (long long) (kResampleTile - 1) * a.M / a.L + 2 * a.half + 1 > kResampleWinFloats)
        kernel_fail("bark-hip: the join takes 1 .. %d ranges, 1 .. 2^25 samples and a table that fits its LDS copy (got R %d, N %d, n_out %d, L %d, M %d, half %d, F %d)",
                    kResampleMaxSegments, a.R, a.N, a.n_out, a.L, a.M, a.half, a.F);
    hipLaunchKernelGGL(join_resample_kernel, dim3((unsigned) ((a.n_out + kResampleTile - 1) / kResampleTile)), dim3(256), 0, s, a);
}

// ---- speaking rate: waveform-similarity overlap-add (rule C16t) -------------------------------------------------------------------
// Frame k's search reads the position frame k - 1 chose, so a segment is one sequential chain of frames: one persistent workgroup per segment, the
// segments of a launch side by side.  Per frame LDS holds the template t[j] = x[pos[k - 1] + 360 + j] (360 floats) and the region x[a - 240 .. a + 240 + 720)
// (1200 floats: the 840 the search reads and 360 more), zero outside the segment; work-item i of 512 runs the chain of candidate i (neighbouring lanes read
// neighbouring LDS words; the template is read four values at a time as a broadcast), an fmaf chain from +0 over j ascending.  No global load sits on the
// chain from frame to frame: the next frame's region depends on k alone and is loaded into registers before this frame's search, and the next template
// x[pos[k] + 360 + j] lies inside this frame's region (winner + 360 + j <= 1199) and is copied from LDS (DESIGN.md section 6 has the times).  The winner is the maximum of the total order (score,
// then scan rank: 0, -1, +1, .., -240, +240 - the first maximum of the rule's scan), which every fold below applies to pairs, so no tree shape changes it:
// xor shuffles inside a wave, eight LDS entries across the waves.  The frame's 360 outputs are formed from the staged
// values - fmaf(w[j], region[winner + j], w[360 + j] * template[j]): one rounded product (the file is built without contraction), one fmaf - and stored
// side by side.  Frame 0 has no search (pos[0] = 0, its template is x[0 .. 360): pos[-1] = -360).
// Where the recording runs past its end: frames whose position + 720 passes n read zeros there, and no frame behind supplies the other half of the
// window, so the last few milliseconds of the output sit lower under the window than the recording does.
// a = floor(360 k p / 1000) is formed in 64 bits (k < 7300, p <= 2000); positions stay below n + 1500 and above -241.
// The window: the f32 roundings of 0.5 - 0.5 cos(2 pi k / 720) formed in double - a committed table, never computed at load time (as kResampleTaps).
static const float kTempoWindow[kTempoFrame] = {
    0.000000000e+00f, 1.903846714e-05f, 7.615242066e-05f, 1.713375095e-04f, 3.045864869e-04f, 4.758892173e-04f, 6.852326333e-04f, 9.326008148e-04f,
    1.217974816e-03f, 1.541333157e-03f, 1.902650925e-03f, 2.301900880e-03f, 2.739052288e-03f, 3.214072203e-03f, 3.726924071e-03f, 4.277569242e-03f,
    4.865965806e-03f, 5.492068361e-03f, 6.155829877e-03f, 6.857199129e-03f, 7.596123498e-03f, 8.372546174e-03f, 9.186408482e-03f, 1.003764756e-02f,
    1.092620008e-02f, 1.185199618e-02f, 1.281496789e-02f, 1.381503977e-02f, 1.485213730e-02f, 1.592618041e-02f, 1.703708619e-02f, 1.818477362e-02f,
    1.936915144e-02f, 2.059013210e-02f, 2.184762247e-02f, 2.314152382e-02f, 2.447174117e-02f, 2.583817206e-02f, 2.724071220e-02f, 2.867925353e-02f,
    3.015368991e-02f, 3.166390583e-02f, 3.320978582e-02f, 3.479121625e-02f, 3.640807420e-02f, 3.806023300e-02f, 3.974757344e-02f, 4.146996140e-02f,
    4.322727025e-02f, 4.501936585e-02f, 4.684610665e-02f, 4.870735854e-02f, 5.060297623e-02f, 5.253281817e-02f, 5.449673906e-02f, 5.649458244e-02f,
    5.852620304e-02f, 6.059144437e-02f, 6.269014627e-02f, 6.482215226e-02f, 6.698729843e-02f, 6.918542087e-02f, 7.141634822e-02f, 7.367991656e-02f,
    7.597595453e-02f, 7.830427587e-02f, 8.066471666e-02f, 8.305709064e-02f, 8.548121154e-02f, 8.793690801e-02f, 9.042397887e-02f, 9.294223785e-02f,
    9.549150616e-02f, 9.807156771e-02f, 1.006822437e-01f, 1.033233330e-01f, 1.059946269e-01f, 1.086959243e-01f, 1.114270166e-01f, 1.141877100e-01f,
    1.169777811e-01f, 1.197970137e-01f, 1.226452067e-01f, 1.255221367e-01f, 1.284275800e-01f, 1.313613355e-01f, 1.343231499e-01f, 1.373128146e-01f,
    1.403301060e-01f, 1.433747709e-01f, 1.464466155e-01f, 1.495453715e-01f, 1.526708156e-01f, 1.558227092e-01f, 1.590008140e-01f, 1.622048914e-01f,
    1.654347032e-01f, 1.686899811e-01f, 1.719704866e-01f, 1.752759814e-01f, 1.786061972e-01f, 1.819608957e-01f, 1.853398085e-01f, 1.887426823e-01f,
    1.921692640e-01f, 1.956192851e-01f, 1.990924925e-01f, 2.025886029e-01f, 2.061073780e-01f, 2.096485198e-01f, 2.132117748e-01f, 2.167968750e-01f,
    2.204035521e-01f, 2.240315080e-01f, 2.276804894e-01f, 2.313501984e-01f, 2.350403666e-01f, 2.387507111e-01f, 2.424809635e-01f, 2.462308258e-01f,
    2.500000000e-01f, 2.537882328e-01f, 2.575951815e-01f, 2.614206076e-01f, 2.652642131e-01f, 2.691257000e-01f, 2.730047405e-01f, 2.769010961e-01f,
    2.808144391e-01f, 2.847444415e-01f, 2.886908650e-01f, 2.926533818e-01f, 2.966316640e-01f, 3.006254733e-01f, 3.046344221e-01f, 3.086582720e-01f,
    3.126966953e-01f, 3.167493939e-01f, 3.208160400e-01f, 3.248963058e-01f, 3.289899230e-01f, 3.330965638e-01f, 3.372159302e-01f, 3.413476646e-01f,
    3.454914987e-01f, 3.496471047e-01f, 3.538141549e-01f, 3.579923213e-01f, 3.621813357e-01f, 3.663808107e-01f, 3.705904782e-01f, 3.748100102e-01f,
    3.790390491e-01f, 3.832773268e-01f, 3.875244856e-01f, 3.917801976e-01f, 3.960441649e-01f, 4.003160298e-01f, 4.045954943e-01f, 4.088822305e-01f,
    4.131759107e-01f, 4.174762070e-01f, 4.217827618e-01f, 4.260953069e-01f, 4.304134548e-01f, 4.347369075e-01f, 4.390653372e-01f, 4.433983862e-01f,
    4.477357566e-01f, 4.520771205e-01f, 4.564221203e-01f, 4.607704580e-01f, 4.651217759e-01f, 4.694757164e-01f, 4.738320112e-01f, 4.781903028e-01f,
    4.825502634e-01f, 4.869115353e-01f, 4.912737906e-01f, 4.956367314e-01f, 5.000000000e-01f, 5.043632388e-01f, 5.087261796e-01f, 5.130884647e-01f,
    5.174497366e-01f, 5.218096972e-01f, 5.261679888e-01f, 5.305242538e-01f, 5.348782539e-01f, 5.392295718e-01f, 5.435778499e-01f, 5.479228497e-01f,
    5.522642136e-01f, 5.566015840e-01f, 5.609346628e-01f, 5.652630925e-01f, 5.695865750e-01f, 5.739046931e-01f, 5.782172084e-01f, 5.825238228e-01f,
    5.868240595e-01f, 5.911177397e-01f, 5.954045057e-01f, 5.996839404e-01f, 6.039558649e-01f, 6.082198024e-01f, 6.124755144e-01f, 6.167227030e-01f,
    6.209609509e-01f, 6.251900196e-01f, 6.294095516e-01f, 6.336191893e-01f, 6.378186941e-01f, 6.420076489e-01f, 6.461858749e-01f, 6.503528953e-01f,
    6.545084715e-01f, 6.586523056e-01f, 6.627840996e-01f, 6.669034362e-01f, 6.710100770e-01f, 6.751036644e-01f, 6.791839600e-01f, 6.832506061e-01f,
    6.873033047e-01f, 6.913416982e-01f, 6.953655481e-01f, 6.993745565e-01f, 7.033683062e-01f, 7.073466182e-01f, 7.113091350e-01f, 7.152555585e-01f,
    7.191855907e-01f, 7.230989337e-01f, 7.269952297e-01f, 7.308743000e-01f, 7.347357869e-01f, 7.385793924e-01f, 7.424048185e-01f, 7.462117672e-01f,
    7.500000000e-01f, 7.537691593e-01f, 7.575190663e-01f, 7.612493038e-01f, 7.649596334e-01f, 7.686498165e-01f, 7.723194957e-01f, 7.759684920e-01f,
    7.795964479e-01f, 7.832031250e-01f, 7.867882252e-01f, 7.903514504e-01f, 7.938926220e-01f, 7.974113822e-01f, 8.009074926e-01f, 8.043807149e-01f,
    8.078307509e-01f, 8.112573028e-01f, 8.146601915e-01f, 8.180391192e-01f, 8.213937879e-01f, 8.247240186e-01f, 8.280295134e-01f, 8.313100338e-01f,
    8.345652819e-01f, 8.377950788e-01f, 8.409991860e-01f, 8.441773057e-01f, 8.473291993e-01f, 8.504546285e-01f, 8.535534143e-01f, 8.566251993e-01f,
    8.596699238e-01f, 8.626871705e-01f, 8.656768799e-01f, 8.686386943e-01f, 8.715724349e-01f, 8.744778633e-01f, 8.773548007e-01f, 8.802030087e-01f,
    8.830222487e-01f, 8.858122826e-01f, 8.885729909e-01f, 8.913040757e-01f, 8.940053582e-01f, 8.966766596e-01f, 8.993177414e-01f, 9.019284248e-01f,
    9.045084715e-01f, 9.070577621e-01f, 9.095759988e-01f, 9.120631218e-01f, 9.145187736e-01f, 9.169428945e-01f, 9.193353057e-01f, 9.216957092e-01f,
    9.240240455e-01f, 9.263200760e-01f, 9.285836220e-01f, 9.308145642e-01f, 9.330127239e-01f, 9.351778626e-01f, 9.373098612e-01f, 9.394085407e-01f,
    9.414737821e-01f, 9.435054064e-01f, 9.455032349e-01f, 9.474672079e-01f, 9.493970275e-01f, 9.512926340e-01f, 9.531539083e-01f, 9.549806118e-01f,
    9.567727447e-01f, 9.585300088e-01f, 9.602524042e-01f, 9.619397521e-01f, 9.635919333e-01f, 9.652087688e-01f, 9.667901993e-01f, 9.683361053e-01f,
    9.698463082e-01f, 9.713207483e-01f, 9.727593064e-01f, 9.741618037e-01f, 9.755282402e-01f, 9.768584967e-01f, 9.781523943e-01f, 9.794098735e-01f,
    9.806308746e-01f, 9.818152189e-01f, 9.829629064e-01f, 9.840738177e-01f, 9.851478338e-01f, 9.861849546e-01f, 9.871850610e-01f, 9.881479740e-01f,
    9.890738130e-01f, 9.899623394e-01f, 9.908136129e-01f, 9.916274548e-01f, 9.924038649e-01f, 9.931427836e-01f, 9.938441515e-01f, 9.945079088e-01f,
    9.951340556e-01f, 9.957224131e-01f, 9.962731004e-01f, 9.967859387e-01f, 9.972609282e-01f, 9.976981282e-01f, 9.980973601e-01f, 9.984586835e-01f,
    9.987820387e-01f, 9.990674257e-01f, 9.993147850e-01f, 9.995241165e-01f, 9.996954203e-01f, 9.998286366e-01f, 9.999238253e-01f, 9.999809861e-01f,
    1.000000000e+00f, 9.999809861e-01f, 9.999238253e-01f, 9.998286366e-01f, 9.996954203e-01f, 9.995241165e-01f, 9.993147850e-01f, 9.990674257e-01f,
    9.987820387e-01f, 9.984586835e-01f, 9.980973601e-01f, 9.976981282e-01f, 9.972609282e-01f, 9.967859387e-01f, 9.962731004e-01f, 9.957224131e-01f,
    9.951340556e-01f, 9.945079088e-01f, 9.938441515e-01f, 9.931427836e-01f, 9.924038649e-01f, 9.916274548e-01f, 9.908136129e-01f, 9.899623394e-01f,
    9.890738130e-01f, 9.881479740e-01f, 9.871850610e-01f, 9.861849546e-01f, 9.851478338e-01f, 9.840738177e-01f, 9.829629064e-01f, 9.818152189e-01f,
    9.806308746e-01f, 9.794098735e-01f, 9.781523943e-01f, 9.768584967e-01f, 9.755282402e-01f, 9.741618037e-01f, 9.727593064e-01f, 9.713207483e-01f,
    9.698463082e-01f, 9.683361053e-01f, 9.667901993e-01f, 9.652087688e-01f, 9.635919333e-01f, 9.619397521e-01f, 9.602524042e-01f, 9.585300088e-01f,
    9.567727447e-01f, 9.549806118e-01f, 9.531539083e-01f, 9.512926340e-01f, 9.493970275e-01f, 9.474672079e-01f, 9.455032349e-01f, 9.435054064e-01f,
    9.414737821e-01f, 9.394085407e-01f, 9.373098612e-01f, 9.351778626e-01f, 9.330127239e-01f, 9.308145642e-01f, 9.285836220e-01f, 9.263200760e-01f,
    9.240240455e-01f, 9.216957092e-01f, 9.193353057e-01f, 9.169428945e-01f, 9.145187736e-01f, 9.120631218e-01f, 9.095759988e-01f, 9.070577621e-01f,
    9.045084715e-01f, 9.019284248e-01f, 8.993177414e-01f, 8.966766596e-01f, 8.940053582e-01f, 8.913040757e-01f, 8.885729909e-01f, 8.858122826e-01f,
    8.830222487e-01f, 8.802030087e-01f, 8.773548007e-01f, 8.744778633e-01f, 8.715724349e-01f, 8.686386943e-01f, 8.656768799e-01f, 8.626871705e-01f,
    8.596699238e-01f, 8.566251993e-01f, 8.535534143e-01f, 8.504546285e-01f, 8.473291993e-01f, 8.441773057e-01f, 8.409991860e-01f, 8.377950788e-01f,
    8.345652819e-01f, 8.313100338e-01f, 8.280295134e-01f, 8.247240186e-01f, 8.213937879e-01f, 8.180391192e-01f, 8.146601915e-01f, 8.112573028e-01f,
    8.078307509e-01f, 8.043807149e-01f, 8.009074926e-01f, 7.974113822e-01f, 7.938926220e-01f, 7.903514504e-01f, 7.867882252e-01f, 7.832031250e-01f,
    7.795964479e-01f, 7.759684920e-01f, 7.723194957e-01f, 7.686498165e-01f, 7.649596334e-01f, 7.612493038e-01f, 7.575190663e-01f, 7.537691593e-01f,
    7.500000000e-01f, 7.462117672e-01f, 7.424048185e-01f, 7.385793924e-01f, 7.347357869e-01f, 7.308743000e-01f, 7.269952297e-01f, 7.230989337e-01f,
    7.191855907e-01f, 7.152555585e-01f, 7.113091350e-01f, 7.073466182e-01f, 7.033683062e-01f, 6.993745565e-01f, 6.953655481e-01f, 6.913416982e-01f,
    6.873033047e-01f, 6.832506061e-01f, 6.791839600e-01f, 6.751036644e-01f, 6.710100770e-01f, 6.669034362e-01f, 6.627840996e-01f, 6.586523056e-01f,
    6.545084715e-01f, 6.503528953e-01f, 6.461858749e-01f, 6.420076489e-01f, 6.378186941e-01f, 6.336191893e-01f, 6.294095516e-01f, 6.251900196e-01f,
    6.209609509e-01f, 6.167227030e-01f, 6.124755144e-01f, 6.082198024e-01f, 6.039558649e-01f, 5.996839404e-01f, 5.954045057e-01f, 5.911177397e-01f,
    5.868240595e-01f, 5.825238228e-01f, 5.782172084e-01f, 5.739046931e-01f, 5.695865750e-01f, 5.652630925e-01f, 5.609346628e-01f, 5.566015840e-01f,
    5.522642136e-01f, 5.479228497e-01f, 5.435778499e-01f, 5.392295718e-01f, 5.348782539e-01f, 5.305242538e-01f, 5.261679888e-01f, 5.218096972e-01f,
    5.174497366e-01f, 5.130884647e-01f, 5.087261796e-01f, 5.043632388e-01f, 5.000000000e-01f, 4.956367314e-01f, 4.912737906e-01f, 4.869115353e-01f,
    4.825502634e-01f, 4.781903028e-01f, 4.738320112e-01f, 4.694757164e-01f, 4.651217759e-01f, 4.607704580e-01f, 4.564221203e-01f, 4.520771205e-01f,
    4.477357566e-01f, 4.433983862e-01f, 4.390653372e-01f, 4.347369075e-01f, 4.304134548e-01f, 4.260953069e-01f, 4.217827618e-01f, 4.174762070e-01f,
    4.131759107e-01f, 4.088822305e-01f, 4.045954943e-01f, 4.003160298e-01f, 3.960441649e-01f, 3.917801976e-01f, 3.875244856e-01f, 3.832773268e-01f,
    3.790390491e-01f, 3.748100102e-01f, 3.705904782e-01f, 3.663808107e-01f, 3.621813357e-01f, 3.579923213e-01f, 3.538141549e-01f, 3.496471047e-01f,
    3.454914987e-01f, 3.413476646e-01f, 3.372159302e-01f, 3.330965638e-01f, 3.289899230e-01f, 3.248963058e-01f, 3.208160400e-01f, 3.167493939e-01f,
    3.126966953e-01f, 3.086582720e-01f, 3.046344221e-01f, 3.006254733e-01f, 2.966316640e-01f, 2.926533818e-01f, 2.886908650e-01f, 2.847444415e-01f,
    2.808144391e-01f, 2.769010961e-01f, 2.730047405e-01f, 2.691257000e-01f, 2.652642131e-01f, 2.614206076e-01f, 2.575951815e-01f, 2.537882328e-01f,
    2.500000000e-01f, 2.462308258e-01f, 2.424809635e-01f, 2.387507111e-01f, 2.350403666e-01f, 2.313501984e-01f, 2.276804894e-01f, 2.240315080e-01f,
    2.204035521e-01f, 2.167968750e-01f, 2.132117748e-01f, 2.096485198e-01f, 2.061073780e-01f, 2.025886029e-01f, 1.990924925e-01f, 1.956192851e-01f,
    1.921692640e-01f, 1.887426823e-01f, 1.853398085e-01f, 1.819608957e-01f, 1.786061972e-01f, 1.752759814e-01f, 1.719704866e-01f, 1.686899811e-01f,
    1.654347032e-01f, 1.622048914e-01f, 1.590008140e-01f, 1.558227092e-01f, 1.526708156e-01f, 1.495453715e-01f, 1.464466155e-01f, 1.433747709e-01f,
    1.403301060e-01f, 1.373128146e-01f, 1.343231499e-01f, 1.313613355e-01f, 1.284275800e-01f, 1.255221367e-01f, 1.226452067e-01f, 1.197970137e-01f,
    1.169777811e-01f, 1.141877100e-01f, 1.114270166e-01f, 1.086959243e-01f, 1.059946269e-01f, 1.033233330e-01f, 1.006822437e-01f, 9.807156771e-02f,
    9.549150616e-02f, 9.294223785e-02f, 9.042397887e-02f, 8.793690801e-02f, 8.548121154e-02f, 8.305709064e-02f, 8.066471666e-02f, 7.830427587e-02f,
    7.597595453e-02f, 7.367991656e-02f, 7.141634822e-02f, 6.918542087e-02f, 6.698729843e-02f, 6.482215226e-02f, 6.269014627e-02f, 6.059144437e-02f,
    5.852620304e-02f, 5.649458244e-02f, 5.449673906e-02f, 5.253281817e-02f, 5.060297623e-02f, 4.870735854e-02f, 4.684610665e-02f, 4.501936585e-02f,
    4.322727025e-02f, 4.146996140e-02f, 3.974757344e-02f, 3.806023300e-02f, 3.640807420e-02f, 3.479121625e-02f, 3.320978582e-02f, 3.166390583e-02f,
    3.015368991e-02f, 2.867925353e-02f, 2.724071220e-02f, 2.583817206e-02f, 2.447174117e-02f, 2.314152382e-02f, 2.184762247e-02f, 2.059013210e-02f,
    1.936915144e-02f, 1.818477362e-02f, 1.703708619e-02f, 1.592618041e-02f, 1.485213730e-02f, 1.381503977e-02f, 1.281496789e-02f, 1.185199618e-02f,
    1.092620008e-02f, 1.003764756e-02f, 9.186408482e-03f, 8.372546174e-03f, 7.596123498e-03f, 6.857199129e-03f, 6.155829877e-03f, 5.492068361e-03f,
    4.865965806e-03f, 4.277569242e-03f, 3.726924071e-03f, 3.214072203e-03f, 2.739052288e-03f, 2.301900880e-03f, 1.902650925e-03f, 1.541333157e-03f,
    1.217974816e-03f, 9.326008148e-04f, 6.852326333e-04f, 4.758892173e-04f, 3.045864869e-04f, 1.713375095e-04f, 7.615242066e-05f, 1.903846714e-05f,
};
const float * tempo_window() { return kTempoWindow; }

__device__ __forceinline__ int tempo_rank(int c) {                      // candidate c = delta + 240 -> its place in the scan 0, -1, +1, -2, +2, ..
    const int d = c - kTempoRadius;
    return d == 0 ? 0 : d < 0 ? -2 * d - 1 : 2 * d;
}
// b before a in the total order: the greater score, then the earlier place in the scan (scores are finite: |x| < 65520)
__device__ __forceinline__ bool tempo_better(float sb, int rb, float sa, int ra) { return sb > sa || (sb == sa && rb < ra); }

constexpr int kTempoThreads = 512, kTempoWide = kTempoCandidates + kTempoFrame - 1;      // the staged region: x[a - 240 .. a + 240 + 720), 1200 floats
static_assert(kTempoThreads >= kTempoHop && 3 * kTempoThreads >= kTempoWide && 2 * kTempoThreads < kTempoWide, "one template value and up to three region values per work-item");
__global__ __launch_bounds__(kTempoThreads) void tempo_kernel(const TempoArgs a) {
    __shared__ float win[kTempoFrame];
    __shared__ float4 tmpl4[kTempoHop / 4];
    __shared__ float reg[kTempoWide];
    __shared__ float red_s[kTempoThreads / 64];
    __shared__ int red_r[kTempoThreads / 64];
    constexpr int S = kResampleMaxSegments + 1, HS = kTempoHop, D = kTempoRadius, T = kTempoThreads;
    const int t = (int) threadIdx.x, s = (int) blockIdx.x;
    const int n = a.seg[s], n_out = a.seg[2 * S + s], p = a.seg[4 * S + s];
    const float * x = a.x + a.seg[S + s];
    float * y = a.y + a.seg[3 * S + s];
    int * pos = a.pos + a.seg[5 * S + s];
    const int K = (n_out + HS - 1) / HS;
    if (p == 1000) {                                                     // the identity by definition: the samples themselves, the nominal positions
        for (int i = t; i < n; i += T) y[i] = x[i];
        for (int k = t; k < K; k += T) pos[k] = k * HS;
        return;
    }
    auto sample = [&](int g) { return (g >= 0 && g < n) ? x[g] : 0.0f; };
    for (int i = t; i < kTempoFrame; i += T) win[i] = a.win[i];
    float * tmpl = reinterpret_cast<float *>(tmpl4);
    const int c0 = t < kTempoCandidates ? t : kTempoCandidates - 1;       // work-items 481 .. 511 run the last candidate once more: the same score and rank
    const int r0 = tempo_rank(c0);
    // frame 0: pos[-1] = -360, so its template is x[0 .. 360); its region lies around a = 0
    if (t < HS) tmpl[t] = sample(t);
    for (int i = t; i < kTempoWide; i += T) reg[i] = sample(i - D);
    int nom = 0;
    for (int k = 0; k < K; k++) {
        // the next frame's region, known before this frame's search ends: loaded now, stored behind the frame (the loads fly while the chains run)
        const bool more = k + 1 < K;
        const int nom1 = (int) ((long long) (k + 1) * HS * p / 1000);
        float f0 = 0.0f, f1 = 0.0f, f2 = 0.0f;
        if (more) {
            f0 = sample(nom1 - D + t); f1 = sample(nom1 - D + t + T);
            if (t + 2 * T < kTempoWide) f2 = sample(nom1 - D + t + 2 * T);
        }
        __syncthreads();
        if (k > 0) {
            const float * q0 = reg + c0;
            float bs = 0.0f;
            for (int q = 0; q < HS / 4; q++) {
                const float4 tv = tmpl4[q];
                bs = fmaf(tv.x, q0[4 * q], bs);
                bs = fmaf(tv.y, q0[4 * q + 1], bs);
                bs = fmaf(tv.z, q0[4 * q + 2], bs);
                bs = fmaf(tv.w, q0[4 * q + 3], bs);
            }
            int br = r0;
            for (int off = 32; off > 0; off >>= 1) {
                const float os = __shfl_xor(bs, off, 64);
                const int orr = __shfl_xor(br, off, 64);
                if (tempo_better(os, orr, bs, br)) { bs = os; br = orr; }
            }
            if ((t & 63) == 0) { red_s[t >> 6] = bs; red_r[t >> 6] = br; }
        }
        __syncthreads();
        int cb = D;                                                      // frame 0: delta = 0
        if (k > 0) {
            float bs = red_s[0]; int br = red_r[0];
            for (int w = 1; w < T / 64; w++) if (tempo_better(red_s[w], red_r[w], bs, br)) { bs = red_s[w]; br = red_r[w]; }
            cb = D + (br == 0 ? 0 : (br & 1) ? -((br + 1) >> 1) : (br >> 1));
        }
        float next_t = 0.0f;                                             // the next template x[pos[k] + 360 + j] lies in this frame's region
        if (t < HS) {
            const int m = k * HS + t;
            if (m < n_out) y[m] = fmaf(win[t], reg[cb + t], win[HS + t] * tmpl[t]);
            next_t = reg[cb + HS + t];
        }
        if (t == 0) pos[k] = nom + cb - D;
        __syncthreads();                                                 // every read of this frame's template and region is done
        if (more) {
            if (t < HS) tmpl[t] = next_t;
            reg[t] = f0; reg[t + T] = f1;
            if (t + 2 * T < kTempoWide) reg[t + 2 * T] = f2;
            nom = nom1;
        }
    }
}
void launch_tempo(hipStream_t s, const TempoArgs & a, const int (&h)[6][kResampleMaxSegments + 1]) {
    bool ok = a.x && a.y && a.win && a.seg && a.pos && a.B >= 1 && a.B <= kResampleMaxSegments && h[1][0] == 0 && h[3][0] == 0 && h[5][0] == 0;
    for (int i = 0; ok && i < a.B; i++) {
        const int n = h[0][i], p = h[4][i];
        ok = n >= 1 && n <= kResampleMaxSamples && p >= kTempoMinSpeed && p <= kTempoMaxSpeed;
        if (!ok) break;
        const int n_out = p == 1000 ? n : (int) ((1000LL * n + p - 1) / p);
        ok = h[2][i] == n_out && h[1][i + 1] == h[1][i] + n && h[3][i + 1] == h[3][i] + n_out && h[5][i + 1] == h[5][i] + (n_out + kTempoHop - 1) / kTempoHop;
    }
    if (!ok) kernel_fail("bark-hip: the time-scale kernel takes 1 .. %d segments of 1 .. %d samples at 500 .. 2000 per mille and a table of prefix sums that follows rule C16t (got B %d)",
                         kResampleMaxSegments, kResampleMaxSamples, a.B);
    hipLaunchKernelGGL(tempo_kernel, dim3((unsigned) a.B), dim3(kTempoThreads), 0, s, a);
}

// ---- loudness (rule C17l) -------------------------------------------------------------------------------------------------------------------------------
// The constants are committed as hexadecimal literals, so no libm decides a bit: the K-weighting prototypes of BS.1770 evaluated at 24 kHz in double
// (tests/loudness_ref.py formulas(), which gives the ITU's 48 kHz table to 9e-16), the absolute gate 10^((-70 + 0.691) / 10) and 9600 times it.
constexpr double kLoudConst[9] = {
    0x1.7ce70764be80ap+0, -0x1.1f83a928e19b5p+1, 0x1.cf503fa464169p-1, -0x1.63e66a4312152p+0, 0x1.12dc7e507ed4ep-1,       // shelf b0, b1, b2, a1, a2
    -0x1.faeab9b7850f0p+0, 0x1.f5e262f9b05f4p-1,                                                                             // high-pass a1, a2
    0x1.f791ec6e1d5b7p-24, 0x1.270f808885339p-10,                                                                            // A, 9600 A
};
const double * loudness_constants() { return kLoudConst; }

// One wave per workgroup: the chain of a lane is 7200 dependent steps, so the waves of a launch should spread over the CUs.  A lane reads 7200 floats that
// lie 2400 floats from its neighbour's: the wave stages a tile of 16 samples per lane through LDS, 16 consecutive work-items fetching the 64 bytes of one
// lane (rows 17 floats apart: the owner's reads are free of bank conflicts), the next tile's loads in flight while the chains of this one run.
constexpr int kLoudLanes = 64, kLoudTile = 16, kLoudRow = kLoudTile + 1, kLoudTiles = kLoudRun / kLoudTile, kLoudPreTiles = kLoudPre / kLoudTile;
static_assert(kLoudRun % kLoudTile == 0 && kLoudPre % kLoudTile == 0 && kLoudLanes % kLoudTile == 0, "whole tiles in the warm-up and in the hop");
__global__ __launch_bounds__(kLoudLanes) void loudness_hops_kernel(const LoudnessArgs a) {
    __shared__ float tile[kLoudLanes * kLoudRow];
    __shared__ long long row_first[kLoudLanes];                          // index into a.x of a lane's step 0 (may lie in front of its segment)
    __shared__ long long row_lo[kLoudLanes], row_hi[kLoudLanes];         // the samples a lane may read: [lo, hi) in a.x, everything else is +0
    constexpr int S = kResampleMaxSegments + 1, R = kLoudLanes / kLoudTile;
    const int t = (int) threadIdx.x;
    const int lane = (int) blockIdx.x * kLoudLanes + t;
    int s = -1, h = 0, Hn = 0;
    if (lane < a.seg[4 * S + a.B]) {
        s = 0;
        while (lane >= a.seg[4 * S + s + 1]) s++;                        // at most 64 steps
        h = lane - a.seg[4 * S + s];
        Hn = a.seg[2 * S + s];
    }
    {
        long long first = 0, lo = 0, hi = 0;                             // a lane without work reads nothing
        if (s >= 0) {
            const long long off = a.seg[S + s];
            first = off + (long long) (h - 2) * kLoudHop;
            if (h < Hn) { lo = off + (long long) (h > 2 ? h - 2 : 0) * kLoudHop; hi = off + (long long) (h + 1) * kLoudHop; }
            else { lo = off + (long long) Hn * kLoudHop; hi = off + a.seg[s]; }      // the samples behind the last hop: their peak alone
        }
        row_first[t] = first; row_lo[t] = lo; row_hi[t] = hi;
    }
    __syncthreads();
    const int col = t % kLoudTile, sub = t / kLoudTile;
    auto fetch = [&](int tl, float (&f)[kLoudTile]) {
#pragma unroll
        for (int i = 0; i < kLoudTile; i++) {
            const int r = i * R + sub;
            const long long g = row_first[r] + (long long) tl * kLoudTile + col;
            f[i] = (g >= row_lo[r] && g < row_hi[r]) ? a.x[g] : 0.0f;
        }
    };
    const double b0 = kLoudConst[0], b1 = kLoudConst[1], b2 = kLoudConst[2], a1 = kLoudConst[3], a2 = kLoudConst[4], ha1 = kLoudConst[5], ha2 = kLoudConst[6];
    double s1 = 0.0, s2 = 0.0, t1 = 0.0, t2 = 0.0, z = 0.0;
    float pk = 0.0f;
    float f[kLoudTile];
    fetch(0, f);
    for (int tl = 0; tl < kLoudTiles; tl++) {
#pragma unroll
        for (int i = 0; i < kLoudTile; i++) tile[(i * R + sub) * kLoudRow + col] = f[i];
        __syncthreads();
        if (tl + 1 < kLoudTiles) fetch(tl + 1, f);
        const bool own = tl >= kLoudPreTiles;                            // the hop's own outputs: the last 2400 steps
#pragma unroll
        for (int i = 0; i < kLoudTile; i++) {
            const float xf = tile[t * kLoudRow + i];
            const double x = (double) xf;
            const double y = b0 * x + s1;                                // shelf
            s1 = (b1 * x - a1 * y) + s2;
            s2 = b2 * x - a2 * y;
            const double y2 = y + t1;                                    // high-pass, b = 1, -2, 1
            t1 = (-2.0 * y - ha1 * y2) + t2;
            t2 = y - ha2 * y2;
            if (own) { z = z + y2 * y2; pk = fmaxf(pk, fabsf(xf)); }
        }
        __syncthreads();                                                 // every read of the tile is done
    }
    if (s >= 0) {
        if (h < Hn) a.z[a.seg[3 * S + s] + h] = z;
        atomicMax(a.peak + s, __builtin_bit_cast(unsigned, pk));         // |x| >= +0: the order of the bits is the order of the values
    }
}

constexpr int kLoudLevelThreads = 256;
__global__ __launch_bounds__(kLoudLevelThreads) void loudness_level_kernel(const LoudnessArgs a) {
    __shared__ float g_sh;
    constexpr int S = kResampleMaxSegments + 1;
    const int t = (int) threadIdx.x, s = (int) blockIdx.x;
    const int n = a.seg[s], Hn = a.seg[2 * S + s];
    if (t == 0) {
        const double * z = a.z + a.seg[3 * S + s];
        const double gate = kLoudConst[8];
        const int J = Hn >= kLoudBlockHops ? Hn - (kLoudBlockHops - 1) : 0;
        int c1 = 0, c2 = 0;
        double sum1 = 0.0, sum2 = 0.0;
        for (int j = 0; j < J; j++) {
            const double Sj = ((z[j] + z[j + 1]) + z[j + 2]) + z[j + 3];
            if (Sj > gate) { c1++; sum1 = sum1 + Sj; }
        }
        const double rel = 0.1 * sum1;
        for (int j = 0; j < J; j++) {
            const double Sj = ((z[j] + z[j + 1]) + z[j + 2]) + z[j + 3];
            if (Sj > gate && Sj * (double) c1 > rel) { c2++; sum2 = sum2 + Sj; }
        }
        const float peak = __builtin_bit_cast(float, a.peak[s]);
        const LoudnessReq rq = a.req[s];
        LoudnessInfo inf;
        inf.mean_square = 0.0; inf.peak = peak; inf.gain = 1.0f; inf.n_blocks = J; inf.n_abs = c1; inf.n_gated = c2; inf.flags = c2 ? 0 : kLoudUnmeasurable;
        if (c2) {
            const double M = sum2 / (9600.0 * (double) c2);
            inf.mean_square = M;
            if (rq.tms > 0.0) {
                double g = sqrt(rq.tms / M);
                if (rq.max_gain > 0.0f && (double) rq.max_gain < g) { g = (double) rq.max_gain; inf.flags |= kLoudCapBound; }
                if (rq.peak_ceiling > 0.0f && peak > 0.0f) {
                    const double lim = (double) rq.peak_ceiling / (double) peak;
                    if (lim < g) { g = lim; inf.flags = (inf.flags & ~kLoudCapBound) | kLoudCeilingBound; }
                }
                inf.gain = (float) g;
            }
        }
        a.info[s] = inf;
        g_sh = inf.gain;
    }
    __syncthreads();
    if (!a.y) return;
    const float g32 = g_sh;
    const float * x = a.x + a.seg[S + s];
    float * y = a.y + a.seg[S + s];
    for (int i = t; i < n; i += kLoudLevelThreads) y[i] = x[i] * g32;
}

void launch_loudness_hops(hipStream_t s, const LoudnessArgs & a, const int (&h)[5][kResampleMaxSegments + 1]) {
    bool ok = a.x && a.seg && a.z && a.peak && a.B >= 1 && a.B <= kResampleMaxSegments && h[1][0] == 0 && h[3][0] == 0 && h[4][0] == 0;
    for (int i = 0; ok && i < a.B; i++) {
        const int n = h[0][i];
        ok = n >= 1 && n <= kResampleMaxSamples && h[2][i] == n / kLoudHop && h[1][i + 1] == h[1][i] + n && h[3][i + 1] == h[3][i] + n / kLoudHop &&
             h[4][i + 1] == h[4][i] + n / kLoudHop + 1;
    }
    if (!ok) kernel_fail("bark-hip: the loudness kernel takes 1 .. %d segments of 1 .. %d samples and a table of prefix sums that follows rule C17l (got B %d)",
                         kResampleMaxSegments, kResampleMaxSamples, a.B);
    hipLaunchKernelGGL(loudness_hops_kernel, dim3((unsigned) ((h[4][a.B] + kLoudLanes - 1) / kLoudLanes)), dim3(kLoudLanes), 0, s, a);
}
void launch_loudness_level(hipStream_t s, const LoudnessArgs & a) {
    if (!a.x || !a.seg || !a.z || !a.peak || !a.req || !a.info || a.B < 1 || a.B > kResampleMaxSegments)
        kernel_fail("bark-hip: the level kernel takes 1 .. %d segments, their z table, peaks and requests (got B %d)", kResampleMaxSegments, a.B);
    hipLaunchKernelGGL(loudness_level_kernel, dim3((unsigned) a.B), dim3(kLoudLevelThreads), 0, s, a);
}

// ---- FLAC (rule C18f) ------------------------------------------------------------------------------------------------------------------------------------
int flac_rate_code(int rate) {
    switch (rate) {
        case 8000: return 4; case 12000: return 12; case 16000: return 5; case 22050: return 6; case 24000: return 7; case 32000: return 8; case 44100: return 9;
        case 48000: return 10; default: return 0;
    }
}

constexpr int kFlacThreads = 256, kFlacWords = kFlacFrameStride / 4;
static_assert(kFlacBlock % kFlacThreads == 0 && kFlacFrameStride % 16 == 0 && (kFlacThreads >> kFlacMaxPartitionOrder) >= 1, "whole samples per lane, aligned slots");

// v (nb bits, 1 .. 32, v < 2^nb) at bit `pos` of a big-endian bit string kept in zeroed LDS words.  The bits of different codes are disjoint, so an add is an
// or: ds_add_u32 without a return value.  A code's neighbours belong to other lanes, so the two words it may touch are shared: hence the atomic.
__device__ __forceinline__ void flac_put(unsigned * w, unsigned pos, unsigned v, int nb) {
    const unsigned i = pos >> 5;
    const int room = 32 - (int) (pos & 31u);
    if (nb <= room) atomicAdd(w + i, v << (room - nb));
    else { atomicAdd(w + i, v >> (nb - room)); atomicAdd(w + i + 1, v << (32 - (nb - room))); }
}
__device__ __forceinline__ unsigned flac_byte(const unsigned * w, int j) { return (w[j >> 2] >> (24 - 8 * (j & 3))) & 0xFFu; }
// a b mod x^16 + x^15 + x^2 + 1 over GF(2), a and b reduced
__device__ __forceinline__ unsigned flac_mulmod16(unsigned a, unsigned b) {
    unsigned r = 0;
    for (int bit = 15; bit >= 0; bit--) {
        r <<= 1;
        if (r & 0x10000u) r ^= 0x18005u;
        if ((b >> bit) & 1u) r ^= a;
    }
    return r;
}
// the FIXED predictor's residual of sample i (i >= order)
__device__ __forceinline__ int flac_residual(const short * s, int i, int order) {
    switch (order) {
        case 0: return s[i];
        case 1: return s[i] - s[i - 1];
        case 2: return s[i] - 2 * s[i - 1] + s[i - 2];
        case 3: return s[i] - 3 * s[i - 1] + 3 * s[i - 2] - s[i - 3];
        default: return s[i] - 4 * s[i - 1] + 6 * s[i - 2] - 4 * s[i - 3] + s[i - 4];
    }
}
// what a frame's choices are, for the lanes that code its samples
struct FlacPlan { int n, order, po, code; };
// Sample i's code: its bit length, and (emit) the bits at `pos`.  FIXED: a warm-up sample in 16 bits, or the residual - behind the residual header and the
// partition's parameter where it is the first of its partition - as q zero bits (skipped: the words are zero), a one and k bits, or raw in the escape width.
template <bool emit>
__device__ __forceinline__ unsigned flac_code(const FlacPlan & p, int i, const short * smp, const unsigned * zz, const unsigned * node_k, const unsigned * node_w,
                                              unsigned * w, unsigned pos) {
    if (p.code == 1 || i < p.order) {
        if (emit) flac_put(w, pos, (unsigned) (unsigned short) smp[i], 16);
        return 16;
    }
    const int psz = p.n >> p.po, part = i / psz, node = (1 << p.po) - 1 + part;
    const unsigned k = node_k[node], wd = node_w[node];
    unsigned len = 0;
    if (i == (part == 0 ? p.order : part * psz)) {
        const int hb = part == 0 ? 10 : 4;                                // coding method 00 and the partition order in front of the first parameter
        if (emit) flac_put(w, pos, ((unsigned) (part == 0 ? p.po : 0) << 4) | k, hb);
        len = (unsigned) hb;
        if (k == 15u) { if (emit) flac_put(w, pos + len, wd, 5); len += 5; }
    }
    const unsigned u = zz[i];
    if (k == 15u) {
        if (emit && wd) flac_put(w, pos + len, ((u >> 1) ^ (0u - (u & 1u))) & (0xFFFFFFFFu >> (32 - wd)), (int) wd);
        return len + wd;
    }
    const unsigned q = u >> k;
    if (emit) flac_put(w, pos + len + q, (1u << k) | (u & ((1u << k) - 1u)), (int) k + 1);
    return len + q + k + 1;
}

__global__ __launch_bounds__(kFlacThreads) void flac_frames_kernel(const FlacArgs a) {
    __shared__ short smp[kFlacBlock];
    __shared__ unsigned zz[kFlacBlock];                                  // the zigzag residuals of the chosen order
    __shared__ unsigned words[kFlacWords];                               // the frame, big-endian bit string
    __shared__ unsigned sums[6];                                         // the five absolute sums, and whether two samples differ
    __shared__ unsigned part_sum[1 << kFlacMaxPartitionOrder][16];       // per finest partition: sum of u >> k for k 0 .. 14, and the largest u
    __shared__ unsigned node_bits[32], node_k[32], node_w[32];           // the partition tree: node (1 << po) - 1 + q is partition q at order po
    __shared__ unsigned scan[kFlacThreads];
    __shared__ int plan_sh[2];
    constexpr int S = kResampleMaxSegments + 1;
    const int t = (int) threadIdx.x, g = (int) blockIdx.x;
    int r = 0;
    while (g >= a.seg[2 * S + r + 1]) r++;                               // at most 64 steps
    const int f = g - a.seg[2 * S + r];
    const int n = min(kFlacBlock, a.seg[r] - f * kFlacBlock);
    const short * x = a.x + a.seg[S + r] + (long long) f * kFlacBlock;
    for (int i = t; i < n; i += kFlacThreads) smp[i] = x[i];
    for (int i = t; i < kFlacWords; i += kFlacThreads) words[i] = 0u;
    if (t < 6) sums[t] = 0u;
    if (t < 16 << kFlacMaxPartitionOrder) part_sum[t >> 4][t & 15] = 0u;
    __syncthreads();
    // the five absolute sums: |r4| <= 2^19 and 4096 of them stay below 2^32
    {
        unsigned acc[5] = {0u, 0u, 0u, 0u, 0u}, differ = 0u;
        for (int i = t; i < n; i += kFlacThreads) {
            differ |= (unsigned) (smp[i] != smp[0]);
#pragma unroll
            for (int o = 0; o < 5; o++) if (i >= o) { const int e = flac_residual(smp, i, o); acc[o] += (unsigned) (e < 0 ? -e : e); }
        }
#pragma unroll
        for (int o = 0; o < 5; o++) atomicAdd(sums + o, acc[o]);
        if (differ) atomicMax(sums + 5, 1u);
    }
    __syncthreads();
    // the frame header: the same for every lane, written by the first
    unsigned char head[12];
    int hn = 0;
    head[hn++] = 0xFF; head[hn++] = 0xF8;
    head[hn++] = (unsigned char) (((n == kFlacBlock ? 12 : 7) << 4) | a.rate_code);
    head[hn++] = 0x08;
    if (f < 0x80) head[hn++] = (unsigned char) f;
    else if (f < 0x800) { head[hn++] = (unsigned char) (0xC0 | (f >> 6)); head[hn++] = (unsigned char) (0x80 | (f & 0x3F)); }
    else { head[hn++] = (unsigned char) (0xE0 | (f >> 12)); head[hn++] = (unsigned char) (0x80 | ((f >> 6) & 0x3F)); head[hn++] = (unsigned char) (0x80 | (f & 0x3F)); }
    if (n != kFlacBlock) { head[hn++] = (unsigned char) ((n - 1) >> 8); head[hn++] = (unsigned char) ((n - 1) & 0xFF); }
    if (a.rate_code == 12) head[hn++] = (unsigned char) a.rate_khz;
    {
        unsigned c = 0;                                                  // CRC-8, x^8 + x^2 + x + 1: ten bytes at most, so the serial form
        for (int j = 0; j < hn; j++) { c ^= head[j]; for (int b = 0; b < 8; b++) c = (c & 0x80u) ? ((c << 1) ^ 0x07u) & 0xFFu : (c << 1) & 0xFFu; }
        head[hn++] = (unsigned char) c;
    }
    if (t == 0) for (int j = 0; j < hn; j++) flac_put(words, 8u * (unsigned) j, head[j], 8);
    const unsigned body_at = 8u * (unsigned) hn + 8u;                    // behind the subframe header
    FlacPlan p{n, 0, 0, 0};
    unsigned total_bits = body_at;
    if (sums[5] == 0u) {                                                 // CONSTANT
        if (t == 0) flac_put(words, body_at, (unsigned) (unsigned short) smp[0], 16);      // (the subframe header is eight zero bits)
        total_bits += 16u;
    } else {
        const int omax = min(4, n - 1);
        for (int o = 1; o <= omax; o++) if (sums[o] < sums[p.order]) p.order = o;
        for (int i = t; i < n; i += kFlacThreads) if (i >= p.order) { const int e = flac_residual(smp, i, p.order); zz[i] = ((unsigned) e << 1) ^ (unsigned) (e >> 31); }
        int P = 0;                                                       // the finest partition order the block size and the order allow
        while (P < kFlacMaxPartitionOrder && n % (2 << P) == 0 && (n >> (P + 1)) > p.order) P++;
        __syncthreads();
        {   // sum of u >> k over every finest partition: kFlacThreads >> P lanes each
            const int T = kFlacThreads >> P, part = t / T, l = t % T, psz = n >> P;
            unsigned acc[15], mx = 0u;
#pragma unroll
            for (int k = 0; k < 15; k++) acc[k] = 0u;
            for (int i = part * psz + l; i < (part + 1) * psz; i += T) if (i >= p.order) {
                const unsigned u = zz[i];
                mx = max(mx, u);
#pragma unroll
                for (int k = 0; k < 15; k++) acc[k] += u >> k;           // the chosen order's sum of u is at most 2^29: no overflow
            }
#pragma unroll
            for (int k = 0; k < 15; k++) atomicAdd(&part_sum[part][k], acc[k]);
            atomicMax(&part_sum[part][15], mx);
        }
        __syncthreads();
        if (t < (2 << P) - 1) {                                          // one lane per node of the partition tree
            int po = 0;
            while ((2 << po) - 1 <= t) po++;
            const int q = t - ((1 << po) - 1), span = 1 << (P - po);
            const unsigned cnt = (unsigned) ((n >> po) - (q == 0 ? p.order : 0));
            unsigned best_k = 0u, best = 0xFFFFFFFFu, mx = 0u;
            for (int j = q * span; j < (q + 1) * span; j++) mx = max(mx, part_sum[j][15]);
            for (int k = 0; k <= kFlacMaxRice; k++) {
                unsigned sq = 0u;
                for (int j = q * span; j < (q + 1) * span; j++) sq += part_sum[j][k];
                const unsigned b = 4u + cnt * (unsigned) (k + 1) + sq;
                if (b < best) { best = b; best_k = (unsigned) k; }
            }
            const unsigned wd = mx ? 32u - (unsigned) __builtin_clz(mx) : 0u;
            const unsigned esc = 9u + cnt * wd;
            if (esc < best) { best = esc; best_k = 15u; }
            node_bits[t] = best; node_k[t] = best_k; node_w[t] = wd;
        }
        __syncthreads();
        if (t == 0) {
            unsigned best = 0xFFFFFFFFu;
            int best_po = 0;
            for (int po = 0; po <= P; po++) {
                unsigned tot = 0u;
                for (int q = 0; q < 1 << po; q++) tot += node_bits[(1 << po) - 1 + q];
                if (tot < best) { best = tot; best_po = po; }
            }
            const bool fixed = 8u + 16u * (unsigned) p.order + 6u + best < 8u + 16u * (unsigned) n;
            plan_sh[0] = fixed ? 8 + p.order : 1; plan_sh[1] = fixed ? best_po : 0;
            flac_put(words, body_at - 8u, (unsigned) plan_sh[0] << 1, 8);
        }
        __syncthreads();
        p.code = plan_sh[0]; p.po = plan_sh[1];
        // every lane codes ceil(n / 256) consecutive samples: their bit lengths, an exclusive scan over the lanes, then the bits
        const int spt = (n + kFlacThreads - 1) / kFlacThreads, i0 = min(n, t * spt), i1 = min(n, i0 + spt);
        unsigned mine = 0u;
        for (int i = i0; i < i1; i++) mine += flac_code<false>(p, i, smp, zz, node_k, node_w, words, 0u);
        scan[t] = mine;
        __syncthreads();
        for (int d = 1; d < kFlacThreads; d <<= 1) {
            const unsigned add = t >= d ? scan[t - d] : 0u;
            __syncthreads();
            scan[t] += add;
            __syncthreads();
        }
        unsigned pos = body_at + scan[t] - mine;
        for (int i = i0; i < i1; i++) pos += flac_code<true>(p, i, smp, zz, node_k, node_w, words, pos);
        total_bits = body_at + scan[kFlacThreads - 1];
    }
    __syncthreads();
    // CRC-16 (x^16 + x^15 + x^2 + 1) of the frame's bytes: every lane takes a run of bytes, bit by bit, and moves its remainder behind the bytes that
    // follow by a multiplication with x^(8 m) - the remainders then add up
    const int nbytes = (int) ((total_bits + 7u) >> 3);
    {
        const int L = (nbytes + kFlacThreads - 1) / kFlacThreads, b0 = min(nbytes, t * L), b1 = min(nbytes, b0 + L);
        unsigned c = 0u;
        for (int j = b0; j < b1; j++) {
            c ^= flac_byte(words, j) << 8;
            for (int b = 0; b < 8; b++) c = (c & 0x8000u) ? ((c << 1) ^ 0x8005u) & 0xFFFFu : (c << 1) & 0xFFFFu;
        }
        unsigned pw = 1u, base = 2u;                                     // x^(8 m), m bytes behind this lane's run
        for (unsigned e = 8u * (unsigned) (nbytes - b1); e && c; e >>= 1) { if (e & 1u) pw = flac_mulmod16(pw, base); base = flac_mulmod16(base, base); }
        scan[t] = c ? flac_mulmod16(c, pw) : 0u;
    }
    __syncthreads();
    for (int d = kFlacThreads / 2; d >= 1; d >>= 1) {
        if (t < d) scan[t] ^= scan[t + d];
        __syncthreads();
    }
    const unsigned crc = scan[0];
    if (t == 0) flac_put(words, 8u * (unsigned) nbytes, crc, 16);
    __syncthreads();
    const int len = nbytes + 2;
    unsigned * slot = a.scratch + (size_t) g * kFlacWords;
    for (int i = t; i < (len + 3) / 4; i += kFlacThreads) slot[i] = __builtin_bswap32(words[i]);
    if (t == 0) {
        a.flen[g] = len;
        a.finfo[4 * g] = p.code; a.finfo[4 * g + 1] = p.po; a.finfo[4 * g + 2] = len; a.finfo[4 * g + 3] = (int) crc;
    }
}

// One workgroup per (result, y of `split`): all of them scan the result's frame lengths chunk by chunk (a chunk is one length per lane, the carry goes from
// chunk to chunk), every y-th frame is copied by the workgroup y: destination words that the frame owns whole are gathered from two aligned source words and
// written as one dword, the up to three bytes at either end byte by byte (the neighbouring frame writes the other bytes of that word).
constexpr int kFlacPackThreads = 256;
__global__ __launch_bounds__(kFlacPackThreads) void flac_pack_kernel(const FlacArgs a) {
    __shared__ unsigned off_sh[kFlacPackThreads], len_sh[kFlacPackThreads];
    __shared__ unsigned stat[3];                                         // bytes of the results in front, largest frame, 0xFFFFFFFF - smallest frame
    constexpr int S = kResampleMaxSegments + 1;
    const int t = (int) threadIdx.x, r = (int) blockIdx.x, y = (int) blockIdx.y, Y = (int) gridDim.y;
    const int f0 = a.seg[2 * S + r], f1 = a.seg[2 * S + r + 1];
    if (t < 3) stat[t] = 0u;
    __syncthreads();
    {
        unsigned before = 0u;
        for (int i = t; i < f0; i += kFlacPackThreads) before += (unsigned) a.flen[i];
        atomicAdd(stat, before);
    }
    __syncthreads();
    unsigned carry = stat[0];
    const unsigned char * src8 = reinterpret_cast<const unsigned char *>(a.scratch);
    for (int c0 = f0; c0 < f1; c0 += kFlacPackThreads) {
        const unsigned mine = c0 + t < f1 ? (unsigned) a.flen[c0 + t] : 0u;
        if (mine) { atomicMax(stat + 1, mine); atomicMax(stat + 2, 0xFFFFFFFFu - mine); }
        off_sh[t] = mine; len_sh[t] = mine;
        __syncthreads();
        for (int d = 1; d < kFlacPackThreads; d <<= 1) {
            const unsigned add = t >= d ? off_sh[t - d] : 0u;
            __syncthreads();
            off_sh[t] += add;
            __syncthreads();
        }
        const int in_chunk = min(kFlacPackThreads, f1 - c0);
        for (int j = 0; j < in_chunk; j++) {
            if ((c0 + j - f0) % Y != y) continue;
            const unsigned len = len_sh[j], D = carry + off_sh[j] - len;
            const size_t src = (size_t) (c0 + j) * kFlacFrameStride;
            const unsigned w0 = D >> 2, nw = ((D + len + 3u) >> 2) - w0;
            for (unsigned q = (unsigned) t; q < nw; q += kFlacPackThreads) {
                const unsigned wb = (w0 + q) * 4u, lo = max(wb, D), hi = min(wb + 4u, D + len);
                if (hi - lo == 4u) {
                    const unsigned so = lo - D, sh = 8u * (so & 3u);
                    const unsigned * sw = a.scratch + (src >> 2) + (so >> 2);
                    const unsigned v = sh ? (sw[0] >> sh) | (sw[1] << (32u - sh)) : sw[0];
                    reinterpret_cast<unsigned *>(a.out)[w0 + q] = v;
                } else {
                    for (unsigned b = lo; b < hi; b++) a.out[b] = src8[src + (b - D)];
                }
            }
        }
        carry += off_sh[kFlacPackThreads - 1];
        __syncthreads();                                                 // the tables are rewritten by the next chunk
    }
    if (y == 0 && t == 0) {
        a.tot[r] = (int) (carry - stat[0]);
        a.tot[kResampleMaxSegments + r] = (int) (0xFFFFFFFFu - stat[2]);
        a.tot[2 * kResampleMaxSegments + r] = (int) stat[1];
    }
}

void launch_flac_frames(hipStream_t s, const FlacArgs & a, const int (&h)[3][kResampleMaxSegments + 1]) {
    bool ok = a.x && a.seg && a.scratch && a.flen && a.finfo && a.B >= 1 && a.B <= kResampleMaxSegments && h[1][0] == 0 && h[2][0] == 0 && a.rate_code >= 4 &&
              a.rate_code <= 12 && a.rate_code != 11 && (a.rate_code != 12 || a.rate_khz == 12);
    for (int i = 0; ok && i < a.B; i++) {
        const int n = h[0][i];
        ok = n >= 1 && n <= kFlacMaxSamples && h[1][i + 1] - h[1][i] == n && h[1][i + 1] > 0 && h[2][i + 1] == h[2][i] + (n + kFlacBlock - 1) / kFlacBlock;
    }
    if (!ok) kernel_fail("bark-hip: the FLAC kernel takes 1 .. %d results of 1 .. %d samples, a supported rate and a table of prefix sums that follows rule C18f (got B %d)",
                         kResampleMaxSegments, kFlacMaxSamples, a.B);
    hipLaunchKernelGGL(flac_frames_kernel, dim3((unsigned) h[2][a.B]), dim3(kFlacThreads), 0, s, a);
}
void launch_flac_pack(hipStream_t s, const FlacArgs & a, int split) {
    if (!a.seg || !a.scratch || !a.flen || !a.out || !a.tot || a.B < 1 || a.B > kResampleMaxSegments || split < 1 || split > 64)
        kernel_fail("bark-hip: the FLAC pack kernel takes 1 .. %d results, their frames and lengths and a split of 1 .. 64 (got B %d, split %d)", kResampleMaxSegments, a.B, split);
    hipLaunchKernelGGL(flac_pack_kernel, dim3((unsigned) a.B, (unsigned) split), dim3(kFlacPackThreads), 0, s, a);
}

}  // namespace barkhip
