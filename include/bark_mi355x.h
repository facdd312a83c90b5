/*
 * bark_mi355x.h - engine extensions of the MI355X-native Bark library (libbark.so).
 *
 * bark.h stays byte-compatible with the reference; everything the reference API cannot express
 * (device selection, stage-level entry points that the parity tests and benchmarks drive,
 * statistics beyond load/eval time) is declared here with plain C types.
 *
 * Each stage-level entry point replaces one internal function of the reference and is what a
 * maintainer would bind if the reference exposed it (file:line cites /root/reference/bark.cpp):
 *
 *   bark_hip_tokenize        bark_tokenize_input                 bark.cpp:622-662
 *   bark_hip_bert_tokenize   bert_tokenize                       bark.cpp:558-620
 *   bark_hip_gpt_eval        bark_eval_encoder_internal          bark.cpp:1586-1643
 *   bark_hip_fine_eval       bark_eval_fine_encoder_internal     bark.cpp:1907-1959
 *   bark_hip_semantic        bark_forward_text_encoder           bark.cpp:1645-1743
 *   bark_hip_coarse          bark_forward_coarse_encoder         bark.cpp:1745-1905
 *   bark_hip_fine            bark_forward_fine_encoder           bark.cpp:1961-2104
 *   bark_hip_codec_decode    encodec_decompress_audio call site  bark.cpp:2143-2167
 *
 * All of them run on the context's HIP stream and block until their result is on the host.
 * Environment (read at bark_load_model):
 *   BARK_HIP_DEVICE=<n>   HIP device ordinal (default: current device)
 *   BARK_HIP_GRAPH=0|1    replay decode steps from a captured hipGraph (default 1)
 *   (the other switches: INTEGRATION.md section 2)
 *
 * Numerics.  Tokenizer, sampling rules and the token ids of the semantic and coarse stages follow the reference's f16-product / f32-accumulate
 * arithmetic in one fixed summation order (bit-exact against the repository's CPU oracle, which restates it).  The fine model's weight products
 * and the codec's convolutions run on the f16 matrix cores in the hardware's own accumulation order: their outputs are bit-exact against the
 * oracle's emulation of that order and WITHIN TOLERANCE of the reference restatement, not bit-equal to it - fine logits within 2.5e-3, >= 98 % of
 * the fine ids identical on the same coarse input, codec SNR >= 55 dB on the same codes (tests/test_order_divergence.py; BARK_HIP_CROSSCHECK=1280
 * keeps the reference restatement on the device).  Parity against ggml itself is unpinned: the reference cannot be built here.
 */
#pragma once
#include "bark.h"

#ifdef __cplusplus
extern "C" {
#endif

/* which GPT: 0 semantic, 1 coarse, 2 fine */
enum bark_hip_model { BARK_HIP_SEMANTIC = 0, BARK_HIP_COARSE = 1, BARK_HIP_FINE = 2 };

/* out[10] = n_layer, n_head, n_embd, block_size, bias, n_in_vocab, n_out_vocab, n_lm_heads, n_wtes, ftype */
BARK_API int bark_hip_hparams(struct bark_context * bctx, int which, int32_t * out10);

/* Replace the generation parameters of a live context (same struct as bark_load_model takes). */
BARK_API void bark_hip_set_params(struct bark_context * bctx, struct bark_context_params params);

/* 513-id semantic prompt for `text`; returns 513 or <0. */
BARK_API int bark_hip_tokenize(struct bark_context * bctx, const char * text, int32_t * out513);
/* raw WordPiece ids (no offset / padding); returns the count. */
BARK_API int bark_hip_bert_tokenize(struct bark_context * bctx, const char * text, int32_t * out, int n_max);

/* One causal-model evaluation (which = 0|1).  n_tokens ids at positions n_past..; with merge_ctx
 * and n_past == 0 the 513-id prompt collapses to 257 rows.  Writes n_out logits of the last row.
 * Returns the new n_past, or -1. */
BARK_API int bark_hip_gpt_eval(struct bark_context * bctx, int which, const int32_t * tokens, int n_tokens,
                               int n_past, int merge_ctx, float * logits);

/* One fine-model forward: tokens [8][1024] codebook-major, codebook nn in 2..7.
 * logits [1024][n_out].  Returns 0 or -1. */
BARK_API int bark_hip_fine_eval(struct bark_context * bctx, const int32_t * tokens_8x1024, int nn, float * logits);

/* Stage loops (sampled on the device: argmax when temp == 0, multinomial otherwise).  Every output buffer comes with its
 * capacity; a result that does not fit fails the call (-1) instead of overrunning the buffer.
 * semantic: prompt513 -> out (capacity ids; eos_trace, when given, holds capacity + 1 floats); returns count or -1.
 * coarse  : semantic ids -> out [T][2] (capacity_rows rows; T = floor(n_semantic * 75 / 49.9 * 2 / 2)); returns T or -1.
 * fine    : coarse [T][2] -> out [T][8] (capacity_rows rows); returns T or -1 (T <= 8192). */
BARK_API int bark_hip_semantic(struct bark_context * bctx, const int32_t * prompt513, int32_t * out, int capacity, float * eos_trace);
BARK_API int bark_hip_coarse(struct bark_context * bctx, const int32_t * semantic, int n_semantic, int32_t * out_Tx2, int capacity_rows);
BARK_API int bark_hip_fine(struct bark_context * bctx, const int32_t * coarse_Tx2, int T, int32_t * out_Tx8, int capacity_rows);
/* The fine stage of n <= 64 utterances with their windows side by side in every forward pass (what bark_hip_generate_batch runs; f16 model
 * files).  Greedy, or device multinomial with ONE std::mt19937 PER UTTERANCE, each seeded with the next draw of the context's generator
 * (as the utterances of bark_hip_generate_batch are: with fine_temp > 0, fine_many(n = 1) is therefore not bark_hip_fine on the same context).  coarse: the utterances' [T_i][2]
 * arrays back to back, out: their [T_i][8] results back to back (capacity_rows >= sum T_i).  Returns sum T_i or -1. */
BARK_API int bark_hip_fine_many(struct bark_context * bctx, const int32_t * coarse_concat, const int * T, int n, int32_t * out_concat, int capacity_rows);

/* EnCodec decode: codes [n_q][T] (time contiguous) -> pcm (capacity floats; 320 * T are produced). Returns samples or -1. */
BARK_API int bark_hip_codec_decode(struct bark_context * bctx, const int32_t * codes, int n_q, int T, float * pcm, int capacity);

/* Test hook: the decoder's batched form, as every lock-step job runs it (one launch per operator for n <= 32 utterances, their rows back to back).
 * codes[i]: [n_q][T[i]] (time contiguous); utterance i's 320 * T[i] samples are written back to back into pcm_concat (capacity floats), bit-identical
 * to n single calls.  Returns 320 * sum T[i], or -1.  Refused before any work: a null argument or matrix, n outside 1 .. 32, capacity below
 * 320 * sum T[i]; then as bark_hip_codec_decode: a T[i] outside 1 .. 4096, n_q outside 1 .. the file's codebook count, a code outside 0 .. 1023. */
BARK_API int bark_hip_codec_decode_many(struct bark_context * bctx, const int32_t * const * codes, const int * T, int n, int n_q, float * pcm_concat, int capacity);

/* Per-layer parity tap of the codec: activation [C][T'] after stage 0 (first conv), 1 (LSTM + skip),
 * 2..5 (the four upsampling blocks).  Returns the element count or -1. */
BARK_API int bark_hip_codec_tap(struct bark_context * bctx, const int32_t * codes, int n_q, int T, int stage, float * out, int capacity);

/* EnCodec encode (the other direction of the codec; the file must carry the SEANet encoder - the converter's files and the `small` / `large`
 * synthetic files do, `toy` / `mini` do not).  Returns 1 if the context's model file holds the encoder, else 0. */
BARK_API int bark_hip_has_codec_encoder(struct bark_context * bctx);
/* pcm: n_samples floats, 24 kHz mono -> codes [n_q][T] (time contiguous, as bark_hip_codec_decode takes them; capacity in ids), greedy residual vector
 * quantisation over the first n_q codebooks (rule C11q).  Returns T = ceil(n_samples / 320), or -1: no encoder in the file,
 * n_samples < 1 or more than 4096 frames, n_q outside 1 .. the file's codebook count, a sample that is not finite or whose f16 image is not
 * (|x| >= 65520: every convolution reads the f16 image of its input), a latent frame with no finite distance to any codebook row (an error, never a
 * code), capacity < n_q * T. */
BARK_API int bark_hip_codec_encode(struct bark_context * bctx, const float * pcm, int n_samples, int n_q, int32_t * codes, int capacity);
/* n <= 32 recordings in one pass (one launch per operator for all of them, as the decoder's batch); recording i's [n_q][T_i] codes back to back in
 * codes_concat, bit-identical to n single calls.  Returns sum T_i or -1. */
BARK_API int bark_hip_codec_encode_many(struct bark_context * bctx, const float * const * pcm, const int * n_samples, int n, int n_q, int32_t * codes_concat, int capacity);
/* Per-layer parity tap of the encoder, one recording: activation [C][T'] after stage 0 (first conv), 1..4 (after each down-sampling conv), 5 (LSTM + skip),
 * 6 (the latent [hidden_dim][T]).  Returns the element count or -1. */
BARK_API int bark_hip_codec_encode_tap(struct bark_context * bctx, const float * pcm, int n_samples, int stage, float * out, int capacity);
/* The latents [sum T_i][hidden_dim] (time-major, the recordings back to back) that the last bark_hip_codec_encode / _many call of this context quantised;
 * valid until the context's next codec call.  Returns the row count, or -1 (none held, capacity in floats too small). */
BARK_API int bark_hip_codec_encode_latents(struct bark_context * bctx, float * out_TxH, int capacity);
/* Time on the context's stream between the first and the last kernel of its last bark_hip_codec_encode / _many call, in microseconds (hipEvents;
 * the uploads in front and the copy of the codes behind are outside); < 0: no call yet. */
BARK_API double bark_hip_codec_encode_device_us(struct bark_context * bctx);
/* Kernel-level hook (tests): latents [T][hidden_dim] -> codes [n_q][T] by the RVQ kernel alone (T <= 65536).  Returns T, or -1: bad shape, or a frame
 * with no finite distance to any codebook row (a NaN or infinite entry). */
BARK_API int bark_hip_rvq_encode(struct bark_context * bctx, const float * latents_TxH, int T, int n_q, int32_t * codes);

/* Semantic tokens from audio (rule C12h): HuBERT's feature encoder, positional convolution and first `output_layer` layers, then the
 * token head (two LSTM layers, a linear layer, argmax) - the third stream of a voice prompt.  The weights come from a file of their own, written by
 * tools/convert_hubert.py.  Load: 0, or -1 with a message (unreadable, truncated, wrong magic, quantised, dimensions the kernels do not take); the context
 * and the clones made AFTERWARDS share the device copy. */
BARK_API int bark_hip_load_semantic_encoder(struct bark_context * bctx, const char * path);
BARK_API int bark_hip_has_semantic_encoder(struct bark_context * bctx);
/* pcm16k: n_samples floats, 16 kHz mono, not normalised -> ids [T], T = (n_samples - 400) / 320 + 1.  Returns T, or -1: no encoder loaded, n_samples < 400,
 * T > 1024 (n_samples > 328 079), a sample that is not finite or whose f16 image is not (|x| >= 65520), capacity < T.  The context stays usable. */
BARK_API int bark_hip_semantic_encode(struct bark_context * bctx, const float * pcm16k, int n_samples, int32_t * ids, int capacity);
/* Parity tap, time-major rows: stage 0 convolution 0 + norm + GELU [T0][C]; 1 end of the conv stack [T][C]; 2 projection [T][H]; 3 hidden_states[0] [T][H];
 * 4 hidden_states[output_layer] [T][H]; 5 logits [T][n_classes].  Returns the element count or -1 (as above; stage outside 0..5; capacity in floats too small). */
BARK_API int bark_hip_semantic_encode_tap(struct bark_context * bctx, const float * pcm16k, int n_samples, int stage, float * out, int capacity);
/* Kernel-level hook (tests): the token head alone on caller rows feats [T][H], T <= 1024 -> ids [T] and, when logits_or_null is given, logits [T][n_classes].
 * Returns T or -1. */
BARK_API int bark_hip_semantic_head(struct bark_context * bctx, const float * feats_TxH, int T, int32_t * ids, float * logits_or_null);
/* Time on the context's stream between the first and the last kernel of its last bark_hip_semantic_encode call, in microseconds (hipEvents); < 0: no call yet. */
BARK_API double bark_hip_semantic_encode_device_us(struct bark_context * bctx);

/* Voice prompts from a recording (rule C13r): the 24 kHz -> 16 kHz resampler between a recording and the semantic encoder, and one call
 * that makes all three streams of a voice prompt.
 * Resampler: ratio 2 / 3, output m at input time 1.5 m, Hann-windowed sinc (cut-off 0.99 of the new Nyquist frequency, 6 zero crossings on either side), two
 * phases of 22 taps, f32, one fmaf chain per output in ascending tap order, samples outside the recording are zero - the filter of voice.resample_24k_to_16k
 * (bark.cpp_amd/voice.py, float64 in numpy's own summation order) under a stated order; the two agree within a few f32 roundings per output, not bit for bit.
 * bark_hip_resample_taps: the committed table, out[22 phase + (j + 10)] = the tap of x[floor(1.5 m) + j], j = -10 .. 11; returns 44.
 * bark_hip_resample_24k_to_16k: n samples -> n_out = (2 n + 2) / 3 samples; returns n_out, or -1: n < 1, n > 1 310 720 (4096 codec frames), a sample that
 * is not finite, capacity < n_out.  Needs neither encoder. */
BARK_API int bark_hip_resample_taps(float * out44);
BARK_API int bark_hip_resample_24k_to_16k(struct bark_context * bctx, const float * pcm24k, int n, float * out16k, int capacity);
/* A recording longer than this (20 s) is used from its LAST 480 000 samples on: every stage reads the end of its history stream, and the limits of both
 * encoders (1024 HuBERT frames, 4096 codec frames) hold by construction. */
#define BARK_HIP_VOICE_AUDIO_MAX_SAMPLES 480000
/* pcm24k: n_samples floats, 24 kHz mono -> semantic ids [*n_semantic] (the used samples through the resampler, then bark_hip_semantic_encode), fine rows
 * [*n_frames][8] (bark_hip_codec_encode with 8 codebooks, time-major) and coarse rows [*n_frames][2] (their first two codebooks); with n the used sample
 * count, *n_semantic = ((2 n + 2) / 3 - 400) / 320 + 1 and *n_frames = ceil(n / 320).  The result has passed the checks of bark_hip_set_voice_prompt.
 * Returns 0, or -1 with a message: no semantic encoder loaded, no codec encoder in the file, n_samples < 599 (fewer than 400 samples at 16 kHz), a sample
 * anywhere in the recording that is not finite or whose f16 image is not, semantic_capacity < *n_semantic or capacity_rows < *n_frames, or a result
 * bark_hip_set_voice_prompt would refuse (a recording too short to leave a history; an id of a token head with more classes than the model's semantic
 * vocabulary).  The context stays usable.  The semantic ids may differ from voice.from_audio's on undecided frames: the two resamplers differ in the last bits. */
BARK_API int bark_hip_voice_from_audio(struct bark_context * bctx, const float * pcm24k, int n_samples, int32_t * semantic, int semantic_capacity,
                                       int32_t * coarse_Tx2, int32_t * fine_Tx8, int capacity_rows, int32_t * n_semantic, int32_t * n_frames);
/* bark_hip_voice_from_audio, then bark_hip_set_voice_prompt with the result; on -1 the context keeps the voice it had. */
BARK_API int bark_hip_set_voice_from_audio(struct bark_context * bctx, const float * pcm24k, int n_samples);
/* Device time (us) of ONE resampler launch over n samples, averaged over `iters` launches (hipEvents on the context's stream).  Returns < 0 on error. */
BARK_API double bark_hip_time_resample(struct bark_context * bctx, int n, int iters);

/* Output rate and sample format (rule C14r): the rational resampler between 24 kHz and 8000, 12000, 16000, 22050, 32000, 44100 or
 * 48000 Hz (24000 on at least one side; rate_in == rate_out == 24000 is the identity: no filter runs), and the formats f32, s16 and G.711 mu-law.
 * With g = gcd(rate_in, rate_out), L = rate_out / g, M = rate_in / g: c = 0.99 min(1, L / M), W = 6 / c, HALF = ceil(W) + 1, 2 HALF taps per phase,
 * h[p][j] = c sinc(c u) cos^2(pi u / (2 W)) for |u| < W else 0, u = p / L - j, j = -HALF + 1 .. HALF - double precision, rounded once to f32 (24000 -> 16000:
 * the committed table of bark_hip_resample_taps).  Output m: base = floor(m M / L), phase = (m M) mod L, one fmaf chain from +0 over x[base + j] h[phase][j]
 * in ascending j, samples outside the recording +0, no renormalisation; n_out = ceil(n L / M).
 * Formats, by definition format(resample_f32(x)): s16 = rintf(y * 32768) (ties to even) clamped to [-32768, 32767] - |y| reaches 1.87 for |x| <= 1, so the
 * clamp is a real case; mu-law from that s16 value s: sign = s < 0 ? 0x80 : 0, mag = min(|s|, 32635) + 132, e = floor(log2 mag) - 7,
 * man = (mag >> (e + 3)) & 15, byte = ~(sign | e << 4 | man) & 0xFF (0 -> 0xFF, -1 -> 0x7F, 32767 -> 0x80, -32768 -> 0x00). */
enum bark_hip_sample_format { BARK_HIP_SAMPLE_F32 = 0, BARK_HIP_SAMPLE_S16 = 1, BARK_HIP_SAMPLE_MULAW = 2 };
/* a container over the s16 samples, not a sample format of its own: a further value of bark_hip_audio_format.sample_format (rule C18f, below) */
enum bark_hip_container_format { BARK_HIP_SAMPLE_FLAC = 3 };
struct bark_hip_audio_format { int32_t sample_rate; int32_t sample_format; };
/* n_out for n samples (n itself for the identity), or -1: an unsupported pair, n < 0.  Needs no context. */
BARK_API int bark_hip_resample_out_len(int n, int rate_in, int rate_out);
/* The pair's table out[p * 2 HALF + (j + HALF - 1)] and lmh = {L, M, HALF}; returns L * 2 HALF, or -1: an unsupported pair, the identity (it has no
 * table), capacity (in floats) too small.  out may be NULL with capacity 0 to read lmh alone (returns the count).  Needs no context. */
BARK_API int bark_hip_resample_table(int rate_in, int rate_out, float * out, int capacity, int32_t lmh[3]);
/* One recording in f32: n samples at rate_in -> n_out samples at rate_out.  Returns n_out, or -1 (the context stays usable): n < 1, n > 1 310 720, a
 * sample that is not finite, an unsupported pair, capacity (in floats) < n_out. */
BARK_API int bark_hip_resample(struct bark_context * bctx, const float * pcm, int n, int rate_in, int rate_out, float * out, int capacity);
/* count <= 64 segments at rate_in in ONE launch -> their results at to->sample_rate in to->sample_format back to back in out_concat, n_out[i] samples each
 * (n_out may be NULL); bit-identical to count single calls.  Returns the bytes written, or -1 as above (also: a format outside 0 .. 2, capacity_bytes too small). */
BARK_API int bark_hip_resample_many(struct bark_context * bctx, const float * const * pcm, const int * n, int count, int rate_in,
                                    const struct bark_hip_audio_format * to, void * out_concat, int capacity_bytes, int32_t * n_out);
/* The last bark_generate_audio result (24 kHz f32, bark_get_audio_data - which stays what it was) in another rate / format: returns the byte count,
 * -(2 + bytes) if capacity_bytes is too small (out may then be NULL), -1 (no audio held, an unsupported format).  bark_hip_batch_audio_as: the same for
 * utterance i of the context's last job (bark_hip_batch_audio stays what it was). */
BARK_API int bark_hip_get_audio_as(struct bark_context * bctx, const struct bark_hip_audio_format * fmt, void * out, int capacity_bytes);
BARK_API int bark_hip_batch_audio_as(struct bark_context * bctx, int i, const struct bark_hip_audio_format * fmt, void * out, int capacity_bytes);
/* Device time (us) of ONE launch of the rational resampler over n samples of one of the 14 pairs with a filter, with the format's epilogue, averaged over
 * `iters` launches (hipEvents on the context's stream).  Returns < 0 on error. */
BARK_API double bark_hip_time_resample_pair(struct bark_context * bctx, int n, int rate_in, int rate_out, int sample_format, int iters);

/* Long-form text (rules C15s and C15j): a text of any length in, one recording out.  A call of this API speaks at most 256 text
 * slots and n_steps_text_encoder semantic steps (about 15 s); a longer text is split into chunks, the chunks run as ONE lock-step job (one weight read
 * per step for all of them) and their audio is joined on the device - trim, fade, gaps, rate and format in two launches.
 *
 * C15s, the splitter.  Whitespace is the six ASCII bytes space \t \n \r \f \v; a word is a maximal run of other bytes; count(span) is what
 * bark_hip_bert_tokenize returns for the span's bytes with n_max = 257 (256 means "over").  A word ends a SENTENCE if, with its trailing closers
 * (" ' ) ] } and U+201D U+2019 U+00BB) stripped, its last byte is . ! or ? or it ends in U+2026, or if the whitespace behind it holds a \n.  It ends a
 * CLAUSE if the stripped last byte is , ; or : or the whole word is - U+2013 or U+2014.  Budget: max_tokens == 0 gives B = 255 and no merging (one
 * sentence per chunk, as Suno's long-form notebook does); 1 <= max_tokens <= 255 gives B = max_tokens with greedy merging; anything else is refused.
 * From word s: extend e word by word while count(s .. e) <= B, E = the last e that fits (a single word over B is a chunk of its own; the tokenizer cuts
 * it as it always did).  E the last word: the chunk is s .. end - without merging the first sentence end in [s, E] still ends it.  Otherwise the cut is
 * a sentence end in [s, E] (the LAST with merging, the FIRST without), else the last clause end in [s, E], else E.  A text without a word gives no chunk;
 * more than 64 chunks is an error.
 * bark_hip_split_text: the chunks of `text` as byte spans spans_Nx2[2 i] = begin, [2 i + 1] = end; returns their count, or -1 (max_tokens outside
 * 0 .. 255, more than 64 chunks, capacity_chunks too small).  Needs no device.
 *
 * C15j, the join.  count <= 64 segments of 24 kHz f32, 1 .. 1 310 720 finite samples each.  Frame j of a segment covers its samples [240 j, min(240 (j + 1), n))
 * and is active iff max |x| >= trim_threshold (0: every frame).  With a, b the first and last active frame the kept range is
 * [240 max(a - trim_pad_frames, 0), min(240 (b + 1 + trim_pad_frames), n)); no active frame: nothing is kept.  Fade: W[k] = (float) (0.5 - 0.5 cos(pi (k + 0.5) / F)),
 * k < F = fade_samples, formed in double and rounded once; sample k of a kept range of length K becomes x * W[d] (one f32 product) where
 * d = min(k, K - 1 - k) < F, and stays x otherwise.  Layout: the kept ranges in order with gap_samples of +0 between consecutive NON-EMPTY ranges, none
 * in front of the first or behind the last: the joined signal J of N <= 2^25 samples.  Result: format(C14r(J, 24000 -> rate)) as defined above for one
 * recording holding J - for the seven other rates and for the identity (24000: no filter); n_out = ceil(N L / M); N == 0 gives 0 bytes.  At most two
 * launches per call whatever the count: one finds the active frames of all segments (not run at threshold 0, where every frame is active), one stages J's samples tile by tile (segment lookup and fade once per staged
 * sample) and runs C14r's chain over them; J itself is never written out for the filtered rates. */
struct bark_hip_join_params {
    int32_t gap_samples;      /* >= 0; default 6000, the notebook's 0.25 s */
    int32_t fade_samples;     /* F, 0 .. 24000; default 0                   */
    float   trim_threshold;   /* >= 0 and finite; 0 = off                   */
    int32_t trim_pad_frames;  /* >= 0                                       */
};
struct bark_hip_long_params { int32_t max_tokens; int32_t chain; struct bark_hip_join_params join; };
BARK_API int bark_hip_split_text(struct bark_context * bctx, const char * text, int max_tokens, int32_t * spans_Nx2, int capacity_chunks);
/* Splits `text` (C15s) and generates every chunk.  NULL pointers take the defaults: long_params {0, 0, {6000, 0, 0, 0}}, the context's parameters
 * with a seed drawn from the context's generator, the context's filter, the context's voice.  chain == 0: all chunks run in ONE
 * bark_hip_generate_batch_voiced job with the given voice; chunk i has seed params->seed + i (wrapping in uint32).  chain == 1: one job per chunk, with
 * the same seeds; chunk i + 1 takes the three token streams of chunk i as its voice (where bark_hip_set_voice_prompt would refuse those - a history too
 * short - it keeps the voice chunk i had).  In both modes chunk i is bit-identical to bark_hip_generate_batch_voiced of that chunk's text alone with
 * that seed, filter and voice.  A text without a word runs as one chunk.  Returns the chunk count, or -1 (a refusal of the splitter, bad join
 * parameters, chain outside 0 .. 1, a chunk that failed: no result is held then).  The results stay with the context until its next long call:
 * bark_hip_long_audio_as: the joined audio (C15j over the chunks' PCM with long_params->join) at fmt's rate and format (NULL: 24000 f32); returns the
 *   byte count, -(2 + bytes) if capacity_bytes is too small (out may then be NULL), -1 (no long result held, an unsupported format).
 * bark_hip_long_chunks: out_Nx4[4 i ..] = text begin, text end, first sample in J, kept samples in J of chunk i; returns the chunk count or -1.
 * bark_hip_long_chunk_audio / _tokens: the untrimmed 24 kHz PCM and the token streams of chunk i, as bark_hip_batch_audio / bark_hip_batch_tokens. */
BARK_API int bark_hip_generate_long(struct bark_context * bctx, const char * text, const struct bark_hip_long_params * long_params,
                                    const struct bark_hip_request_params * params, const struct bark_hip_sampling_filter * filter,
                                    const struct bark_hip_voice_prompt * voice);
BARK_API int bark_hip_long_audio_as(struct bark_context * bctx, const struct bark_hip_audio_format * fmt, void * out, int capacity_bytes);
BARK_API int bark_hip_long_chunks(struct bark_context * bctx, int32_t * out_Nx4, int capacity_chunks);
BARK_API int bark_hip_long_chunk_audio(struct bark_context * bctx, int i, float ** data);
BARK_API int bark_hip_long_chunk_tokens(struct bark_context * bctx, int i, int stage, int32_t * out, int capacity);
/* The join alone (C15j) on caller audio: pcm[i] holds n[i] samples at 24 kHz.  params == NULL: {6000, 0, 0, 0}; to == NULL: 24000 f32.
 * layout_Nx2 (optional): first sample in J and kept samples of every segment (an empty range sits where the next one starts).  Returns the bytes
 * written (0: every segment was trimmed away), -(2 + bytes) if capacity_bytes is too small (out may then be NULL; layout_Nx2 is filled), or -1 with the
 * context still usable: count outside 1 .. 64, n[i] outside 1 .. 1 310 720, a sample that is not finite, an unsupported rate or format, a negative gap,
 * fade or pad, a fade above 24000, a threshold that is negative or not finite, N above 2^25. */
BARK_API int bark_hip_join_many(struct bark_context * bctx, const float * const * pcm, const int * n, int count, const struct bark_hip_join_params * params,
                                const struct bark_hip_audio_format * to, void * out, int capacity_bytes, int32_t * layout_Nx2);
/* Device time (us) of ONE join over `count` segments of n_each samples with the default parameters - the join launch, which is all such a call runs (see
 * above: no activity launch at threshold 0) - averaged over `iters` launches (hipEvents on the context's stream).  bark_hip_time_join_activity: what a
 * threshold adds in front, timed apart: the activity table's fill and the activity launch over the same segments with every frame active.  < 0 on error. */
BARK_API double bark_hip_time_join(struct bark_context * bctx, int count, int n_each, int rate_out, int sample_format, int iters);
BARK_API double bark_hip_time_join_activity(struct bark_context * bctx, int count, int n_each, int iters);

/* Speaking rate (rule C16t): time-scale modification of 24 kHz f32 audio on the device by waveform-similarity overlap-add - the
 * duration changes, the pitch does not.  speed_permille p is an integer in 500 .. 2000 (2000: twice as fast); p == 1000 is the identity bit for bit and
 * runs nothing.  n samples (1 .. 1 310 720, finite, |x| < 65520) give n_out = ceil(1000 n / p) samples in K = ceil(n_out / 360) frames of 720 samples
 * (30 ms) hopped by 360.  Frame k >= 1 searches the 481 positions within +-240 samples (10 ms) of floor(360 k p / 1000) for the best continuation of frame
 * k - 1: one fmaf chain of 360 terms per position, scanned 0, -1, +1, .., -240, +240, a later one wins only with a strictly greater score (silence stays
 * nominal).  y[360 k + j] = fmaf(w[j], x[pos[k] + j], w[360 + j] * x[pos[k - 1] + 360 + j]) with the committed Hann table w and x = +0 outside the
 * recording; the last few milliseconds may sit lower under the window.  Another rate or format is by definition format(C14r(C16t(x), 24000 -> rate)).
 * Long form: the join (C15j) runs over the time-scaled chunks, its gap, fade, threshold and pad as given (in output samples, not scaled).
 * bark_hip_tempo_out_len: n_out, or -1 (n or p out of range); needs no context.  bark_hip_tempo_window: the committed table; returns 720.
 * bark_hip_tempo: returns n_out, or -1 with the context still usable (n, p or a sample out of range, capacity (in floats) too small).
 * bark_hip_tempo_many: count <= 64 segments with a speed each in ONE tempo launch, then the resampler / format launches of bark_hip_resample_many for `to`
 * (NULL: 24000 f32); bit-identical to `count` single calls; n_out (optional): samples per segment; returns the bytes written, or -1.
 * bark_hip_tempo_positions: the K chosen positions pos[k] of a recording (k 360 at p == 1000); returns K, or -1. */
BARK_API int bark_hip_tempo_out_len(int n, int speed_permille);
BARK_API int bark_hip_tempo_window(float * out720);
BARK_API int bark_hip_tempo(struct bark_context * bctx, const float * pcm, int n, int speed_permille, float * out, int capacity);
BARK_API int bark_hip_tempo_many(struct bark_context * bctx, const float * const * pcm, const int * n, int count, const int32_t * speed_permille,
                                 const struct bark_hip_audio_format * to, void * out_concat, int capacity_bytes, int32_t * n_out);
BARK_API int bark_hip_tempo_positions(struct bark_context * bctx, const float * pcm, int n, int speed_permille, int32_t * pos, int capacity);
/* The results a context holds, at a speaking rate: the return conventions of bark_hip_get_audio_as / _batch_audio_as / _long_audio_as (-(2 + bytes) if
 * capacity_bytes is too small, -1 also for a speed outside 500 .. 2000).  speed_permille == 1000: the bytes of the _as form, no further launch.
 * bark_hip_long_audio_at is bark_hip_join_many over the bark_hip_tempo of every chunk. */
BARK_API int bark_hip_get_audio_at(struct bark_context * bctx, const struct bark_hip_audio_format * fmt, int speed_permille, void * out, int capacity_bytes);
BARK_API int bark_hip_batch_audio_at(struct bark_context * bctx, int i, const struct bark_hip_audio_format * fmt, int speed_permille, void * out, int capacity_bytes);
BARK_API int bark_hip_long_audio_at(struct bark_context * bctx, const struct bark_hip_audio_format * fmt, int speed_permille, void * out, int capacity_bytes);
/* Device time (us) of ONE tempo launch over `count` segments of n_each samples at speed_permille (not 1000), averaged over `iters` launches (hipEvents on
 * the context's stream).  Returns < 0 on error. */
BARK_API double bark_hip_time_tempo(struct bark_context * bctx, int count, int n_each, int speed_permille, int iters);

/* Loudness (rule C17l): the integrated loudness of 24 kHz f32 audio by ITU-R BS.1770 with both gates, measured on the device, and one
 * gain per recording that brings it to a target.  Arithmetic: f64, every product and sum rounded once; the K-weighting biquads (BS.1770's prototypes
 * evaluated at 24 kHz) run per 100 ms hop over the 7200 samples that end with the hop, from zero state, and z[h] is the sum of squares of the hop's own 2400
 * outputs; 400 ms blocks S[j] = ((z[j] + z[j+1]) + z[j+2]) + z[j+3]; absolute gate S[j] > 9600 A, relative gate S[j] c1 > 0.1 sum1 (-10 LU), all in the
 * mean-square domain; M = sum2 / (9600 c2).  Fewer than 4 hops (n < 9600) or no block behind the gates: unmeasurable, the gain is exactly 1 and flags has
 * BARK_HIP_LOUDNESS_UNMEASURABLE.  Otherwise g = sqrt(Tms / M), at most max_gain (if > 0), at most peak_ceiling / peak (if both > 0), g32 = (float) g and
 * y[i] = x[i] g32.  The samples obey the tempo calls' limits (1 .. 1 310 720, finite, |x| < 65520).
 * target_centilufs: hundredths of a LUFS, -4000 .. -500; 0: off.  peak_ceiling, max_gain: >= 0 and finite; 0: none.
 * info: mean_square M (0 if unmeasurable), lufs = -0.691 + 10 log10(M) formed on the host (-inf if unmeasurable), peak = max |x|, the gain applied (1
 * where the request is off), n_blocks J, n_abs c1, n_gated c2, flags.
 * bark_hip_loudness_constants: out9 = shelf b0, b1, b2, a1, a2, high-pass a1, a2, A, 9600 A (committed bit patterns); returns 9.  bark_hip_loudness_target_ms:
 * Tms = 10^((t / 100 + 0.691) / 10), or -1 for a target outside the range.  Both need no context.
 * bark_hip_loudness_many: measures count <= 64 recordings in the two launches (no scaled copy); params (NULL: none) only decide the gain that info reports.
 * Returns count, or -1 with the context still usable.  bark_hip_loudness_hops: the z table of one recording; returns Hn = n / 2400, or -1.
 * bark_hip_level_many: caller audio, a request and a speed (NULL: 1000 each) per recording -> level, C16t, `to` (NULL: 24000 f32) in one call without a round
 * trip to the host in between; n_out, info optional; returns the bytes written, or -1.  Every request off: bark_hip_tempo_many itself. */
enum { BARK_HIP_LOUDNESS_UNMEASURABLE = 1, BARK_HIP_LOUDNESS_CAP_BOUND = 2, BARK_HIP_LOUDNESS_CEILING_BOUND = 4 };
struct bark_hip_loudness_params { int32_t target_centilufs; float peak_ceiling; float max_gain; };
struct bark_hip_loudness_info { double mean_square, lufs; float peak, gain; int32_t n_blocks, n_abs, n_gated, flags; };
/* how a held result is rendered: rate and format, speaking rate (1000: none), levelling (target 0: none) */
struct bark_hip_audio_render { struct bark_hip_audio_format fmt; int32_t speed_permille; struct bark_hip_loudness_params loudness; };
BARK_API int bark_hip_loudness_constants(double * out9);
BARK_API double bark_hip_loudness_target_ms(int target_centilufs);
BARK_API int bark_hip_loudness_many(struct bark_context * bctx, const float * const * pcm, const int * n, int count, const struct bark_hip_loudness_params * params,
                                    struct bark_hip_loudness_info * info);
BARK_API int bark_hip_loudness_hops(struct bark_context * bctx, const float * pcm, int n, double * z, int capacity);
BARK_API int bark_hip_level_many(struct bark_context * bctx, const float * const * pcm, const int * n, int count, const struct bark_hip_loudness_params * params,
                                 const int32_t * speed_permille, const struct bark_hip_audio_format * to, void * out_concat, int capacity_bytes, int32_t * n_out,
                                 struct bark_hip_loudness_info * info);
/* The results a context holds, levelled, at a speaking rate, in a format: the return conventions of the _at forms (-1 also for a target outside the range
 * or a negative or non-finite ceiling or cap) and info (optional): one record, for bark_hip_long_audio_with one per chunk (info_capacity records; fewer
 * than the chunks: -1).  Loudness off: the bytes of the _at form, no further launch, info {gain 1, all else 0}.  A long text's chunks are levelled each
 * on its own, untrimmed, in front of tempo and join: the join's threshold sees the levelled signal. */
BARK_API int bark_hip_get_audio_with(struct bark_context * bctx, const struct bark_hip_audio_render * how, void * out, int capacity_bytes, struct bark_hip_loudness_info * info);
BARK_API int bark_hip_batch_audio_with(struct bark_context * bctx, int i, const struct bark_hip_audio_render * how, void * out, int capacity_bytes,
                                       struct bark_hip_loudness_info * info);
BARK_API int bark_hip_long_audio_with(struct bark_context * bctx, const struct bark_hip_audio_render * how, void * out, int capacity_bytes,
                                      struct bark_hip_loudness_info * info, int info_capacity);
/* Device time (us) of ONE loudness_hops launch (level == 0) or ONE loudness_level launch with its scaled copy (level != 0) over `count` segments of n_each
 * samples, averaged over `iters` launches (hipEvents on the context's stream).  Returns < 0 on error. */
BARK_API double bark_hip_time_loudness(struct bark_context * bctx, int count, int n_each, int level, int iters);

/* FLAC (rule C18f): BARK_HIP_SAMPLE_FLAC is a lossless container over the mono s16 samples the format epilogue writes - behind loudness,
 * speaking rate and output rate - encoded on the device in two launches whatever the number of results.  Blocks of 4096 samples (the last frame holds the
 * rest, its size in the header's 16-bit field); fixed block size strategy; per frame one subframe: CONSTANT if all samples are equal, else the FIXED predictor
 * of order 0 .. min(4, n - 1) with the smallest sum of |residual| (ties: the lower order), VERBATIM if that would not be smaller; no wasted-bits detection.
 * Residuals: 4-bit Rice parameters, partition order 0 .. 4 (only orders that divide the block size and leave the first partition longer than the predictor
 * order), per partition the parameter 0 .. 14 with the fewest bits (ties: the lower), the escape code where strictly smaller (raw width: the minimum signed
 * width of the partition's residuals, 0 if all are zero), per frame the partition order with the fewest bits (ties: the lower).  The stream is "fLaC", one
 * STREAMINFO block marked last (block sizes 4096 / 4096, smallest and largest frame, rate, 1 channel, 16 bits, the sample count, MD5 all zeros: not computed),
 * then the frames.  Decoding returns the s16 samples bit for bit.
 * Routes: bark_hip_get_audio_as / _at / _with, bark_hip_batch_audio_as / _at / _with, bark_hip_long_audio_as / _at / _with (one stream over the joined
 * audio) and the collector's submit calls take the format and return a complete stream.  Its length is known only once it is made: these calls render first,
 * then return the byte count, or -(2 + bytes) if capacity_bytes is too small (out may then be NULL).  The calls on caller audio (bark_hip_resample_many,
 * bark_hip_tempo_many, bark_hip_level_many, bark_hip_join_many) keep refusing it: bark_hip_flac_encode_many is the call for caller audio.
 * bark_hip_flac_max_bytes: 42 + 14 ceil(n / 4096) + 2 n, the size no stream of n samples exceeds, or -1 (n outside 1 .. 2^26); needs no context.
 * bark_hip_flac_encode_many: count <= 64 recordings of n[i] s16 samples at `rate` (one of the eight rates) -> their streams back to back in `out`,
 *   lengths[i] (optional) bytes each; returns the bytes written, -(2 + bytes) if capacity_bytes is too small (out may then be NULL; lengths is filled),
 *   or -1 with the context still usable (a null argument, count outside 1 .. 64, n[i] outside 1 .. 2^26, an unsupported rate) before any launch.
 * bark_hip_flac_frames (tests): out_Nx4[4 f ..] = subframe code (0 CONSTANT, 1 VERBATIM, 8 + o FIXED of order o), partition order, byte length and CRC-16 of
 *   frame f of one recording; returns the frame count, or -1 (capacity_frames too small, or what bark_hip_flac_encode_many refuses).
 * bark_hip_time_flac: device time (us) of ONE pair of launches (frames, pack) over `count` recordings of n_each samples (1 .. 1 310 720) of a synthetic
 *   voiced signal at 24 kHz, averaged over `iters` pairs (hipEvents on the context's stream); bark_hip_time_flac_launch: of the frames launch (which == 1)
 *   or the pack launch (which == 2) alone.  < 0 on error.
 * Out of scope: LPC subframes, stereo, 24 bits, seek tables, Vorbis comments, the MD5 signature, streaming delivery. */
BARK_API int bark_hip_flac_max_bytes(int n);
BARK_API int bark_hip_flac_encode_many(struct bark_context * bctx, const int16_t * const * pcm, const int * n, int count, int rate, void * out, int capacity_bytes,
                                       int32_t * lengths);
BARK_API int bark_hip_flac_frames(struct bark_context * bctx, const int16_t * pcm, int n, int rate, int32_t * out_Nx4, int capacity_frames);
BARK_API double bark_hip_time_flac(struct bark_context * bctx, int count, int n_each, int iters);
BARK_API double bark_hip_time_flac_launch(struct bark_context * bctx, int count, int n_each, int which, int iters);

/* Replicas on one GPU: a clone shares the (immutable) device weights of `src` and owns its stream, KV caches and
 * scratch, so several utterances can be in flight on one device.  Free clones and the original in any order. */
BARK_API struct bark_context * bark_hip_clone_context(struct bark_context * src, uint32_t seed);

/* Runs bark_generate_audio for n (context, text) pairs concurrently, one host thread + one HIP stream each
 * (no collectives: utterances are independent).  Returns the number of successful generations; results are read
 * from each context with bark_get_audio_data[_size]. */
BARK_API int bark_hip_generate_audio_batch(struct bark_context ** ctxs, const char * const * texts, int n);

/* In-engine batching: a job of n utterances (n <= 4096) travels through the lock-step slots of ONE context (up to 64; the first call or
 * bark_hip_reserve_batch fixes the number): the live slots advance together through the semantic and coarse decode loops, so every decode
 * kernel reads the weights once per step for all of them; a slot whose utterance has finished (its own step cap / stop rule, its own number
 * of coarse windows) is handed to the next waiting utterance, and when nobody waits the batch is compacted, so no lock step is spent on a
 * finished utterance.  The prompts of the slots go through the model in one pass, the fine windows of 8 utterances side by side, the codec
 * of the utterances in one pass.  Per-utterance results are bit-identical to bark_generate_audio on a fresh context with the same
 * parameters, whatever the job size, the slot count or the company an utterance travels in.  With temp > 0 every
 * utterance has its own std::mt19937 (the reference seeds one per context, bark.cpp:1179): utterance i is what a context
 * loaded with seed seeds[i] would generate; the unseeded call draws those seeds from the context's generator, in order.
 * Every weight format takes this route: f16 files on the matrix cores, q4_0 .. q8_0 and f32 files on per-slot VALU products (f32: every weight
 * chunk is read once for a group of eight slots); for those the prompts go slot by slot and the fine passes utterance by utterance.
 * BARK_HIP_HOST_SAMPLING, and semantic / coarse models of unequal width, degrade the call to a sequential loop (bark_hip_batch_lock_steps tells).
 * Returns the number of utterances that produced audio.  Results: bark_hip_batch_audio / bark_hip_batch_tokens. */
BARK_API int bark_hip_generate_batch(struct bark_context * bctx, const char * const * texts, int n);
BARK_API int bark_hip_generate_batch_seeded(struct bark_context * bctx, const char * const * texts, int n, const uint32_t * seeds);
/* The same with per-utterance parameters - the fields of bark_context_params a request may set for itself (the loops they steer:
 * bark.cpp:1669-1695 step cap and stop rule, :201-247 temperatures); everything else comes from the context.  A server mixes
 * requests with different settings in one job; tests make slots stop at chosen steps. */
struct bark_hip_request_params {
    float    temp;                  /* semantic / coarse sampling temperature, 0 = greedy (bark_context_params::temp)  */
    float    fine_temp;             /* fine sampling temperature, 0 = greedy                                           */
    float    min_eos_p;             /* stop rule of the semantic loop                                                  */
    int32_t  n_steps_text_encoder;  /* step cap of the semantic loop                                                   */
    uint32_t seed;                  /* seed of the utterance's own std::mt19937 (temp > 0 / fine_temp > 0)             */
};
BARK_API int bark_hip_generate_batch_ex(struct bark_context * bctx, const char * const * texts, int n, const struct bark_hip_request_params * per_utterance);

/* Top-k and nucleus (top-p) filtering of the semantic and coarse samples (rule C8n; the semantics of generate_text_semantic /
 * generate_coarse in suno-ai/bark generation.py): top-p on the UNtempered logits first - the ids in descending logit order (ties: ascending id) stay
 * while the weight in front of them is <= top_p of the total (the id that crosses top_p stays, and so does the first); then top-k - survivors below
 * the top_k-th largest surviving logit go (ties with it stay); then temperature and the multinomial draw as before, one uniform draw per sample.
 * Greedy stages (temp 0) and the fine stage are not filtered.  {0, 1.0f} is off: the same kernels, graphs and bits as without a filter. */
struct bark_hip_sampling_filter {
    int32_t top_k;                  /* keep the top_k largest logits, 0 = off            */
    float   top_p;                  /* nucleus mass in (0, 1], 1 = off                   */
};
/* The context's filter for bark_generate_audio, bark_hip_semantic / bark_hip_coarse and the jobs that carry no filters of their own.  Returns 0, or -1
 * for top_k < 0 or top_p outside (0, 1] (NaN included).  bark_hip_clone_context copies it. */
BARK_API int bark_hip_set_sampling_filter(struct bark_context * bctx, int32_t top_k, float top_p);
/* bark_hip_generate_batch_ex with a filter per utterance (filters == NULL: the context's filter for everyone; per_utterance == NULL: the context's
 * parameters).  Every utterance is bit-identical to a fresh context with its parameters, seed and filter. */
BARK_API int bark_hip_generate_batch_filtered(struct bark_context * bctx, const char * const * texts, int n, const struct bark_hip_request_params * per_utterance,
                                              const struct bark_hip_sampling_filter * filters);
/* Voice prompts (speaker history; rule C10v; suno-ai/bark generation.py `history_prompt`): the token streams of an earlier
 * utterance of the speaker, which the three stage loops continue from.  All arrays are time-major, as every [T][2] / [T][8] array of this API
 * (Suno's .npz presets are codebook-major: bark.cpp_amd/voice.py transposes).  semantic ids in [0, semantic_vocab_size), coarse and fine ids in
 * [0, codebook_size).  With r = coarse_rate_hz / semantic_rate_hz * n_coarse_codebooks:
 *   semantic  ids 256..511 of the 513-id prompt are the LAST min(n_semantic, 256) history ids, right-padded with semantic_pad_token;
 *   coarse    n_sh = min(floor(max_coarse_history / r), n_semantic - n_semantic % 2, floor(2 n_coarse_frames / r)), n_ch = round(n_sh r): the last
 *             n_sh semantic ids go in front of the semantic input (semantic_idx = n_sh + round(step_idx / r)), the last n_ch interleaved coarse ids
 *             minus their last TWO in front of the generated ones; step count, window count, codebook parity and the result: the NEW ids only;
 *   fine      the LAST min(n_fine_frames, 512) history rows (all 8 codebooks) go in front of the coarse rows; windows of 1024 rows with a hop of
 *             512 fill from the first new row on; the result is the new rows;
 *   codec     sees the new frames only.
 * bark_hip_set_voice_prompt copies the arrays; NULL clears.  Returns 0, or -1 for ids out of range, a history whose trimmed form is empty (n_sh < 2 or
 * n_ch <= 2) or a history that does not fit the coarse context with the context's window parameters (257 + min(max_coarse_history, n_ch - 2) +
 * sliding_window_size - 1 rows).  It steers bark_generate_audio, bark_hip_tokenize (ids 256..511), bark_hip_coarse, bark_hip_fine, bark_hip_fine_many
 * and the jobs / collector requests that carry no voice of their own; bark_hip_semantic keeps taking the prompt it is given.  bark_hip_clone_context
 * copies it.  No voice prompt: the same kernels, graphs and bits as before. */
struct bark_hip_voice_prompt {
    const int32_t * semantic;   int32_t n_semantic;        /* [n_semantic]            */
    const int32_t * coarse_Tx2; int32_t n_coarse_frames;   /* [n_coarse_frames][2]    */
    const int32_t * fine_Tx8;   int32_t n_fine_frames;     /* [n_fine_frames][8]      */
};
BARK_API int bark_hip_set_voice_prompt(struct bark_context * bctx, const struct bark_hip_voice_prompt * voice);
/* bark_hip_generate_batch_filtered with a voice per utterance (voices == NULL or voices[i] == NULL: the context's).  Every utterance is bit-identical
 * to a fresh context with its parameters, seed, filter and voice under an equal fine order, whatever company it travels in. */
BARK_API int bark_hip_generate_batch_voiced(struct bark_context * bctx, const char * const * texts, int n, const struct bark_hip_request_params * per_utterance,
                                            const struct bark_hip_sampling_filter * filters, const struct bark_hip_voice_prompt * const * voices);
/* Kernel-level hook of the fine stage's pick kernels (tests): n_windows * 1024 rows of n_cols (<= 1024) logits; temp == 0: the greedy pick, else the
 * multinomial pick with the uniform draw u[row].  tokens_io [n_windows * 1024] is the token plane: row z * 1024 + j receives its pick when
 * j >= rel[z] and keeps its value otherwise.  *near_ties (optional): picks settled by the exact path.  Returns 0 or -1. */
BARK_API int bark_hip_pick_rows(struct bark_context * bctx, const float * logits, int n_windows, int n_cols, float temp, const double * u,
                                const int32_t * rel, int32_t * tokens_io, int32_t * near_ties);
/* Fixes the number of lock-step slots (1..64; at least 8 are allocated) before the first job; returns 0 or -1. */
BARK_API int bark_hip_reserve_batch(struct bark_context * bctx, int slots);
/* The lock steps the context's last job ran: out2[0] in the semantic stage, out2[1] in the coarse stage (one lock step = one decode step of all live
 * slots together).  {0, 0}: the sequential fallback served the job.  Returns 0, or -1 when no job has run on the context (out2 untouched). */
BARK_API int bark_hip_batch_lock_steps(struct bark_context * bctx, int32_t out2[2]);
/* audio of utterance i of the last batch: returns the sample count (-1 on error), *data points into the context */
BARK_API int bark_hip_batch_audio(struct bark_context * bctx, int i, float ** data);
/* token stream of utterance i: stage 0 semantic, 1 coarse [T][2], 2 fine [T][8]; returns the id count or -1 */
BARK_API int bark_hip_batch_tokens(struct bark_context * bctx, int i, int stage, int32_t * out, int capacity);

/* Request collector in front of bark_hip_generate_batch - what a server puts where the reference's example holds one mutex around
 * bark_generate_audio (examples/server/server.cpp:76-94,128-163).  Any number of host threads submit; one worker thread owns `bctx`
 * (nobody else may use it while the batcher lives), collects pending requests - up to max_batch (<= 256; the context's slots, at most 64,
 * serve them as one job), waiting at most max_wait_ms
 * for a batch to fill once one request is pending - and runs them as ONE lock-step batch.  A request's result is what a fresh context
 * seeded with its `seed` generates, whatever batch it travelled in (seed is irrelevant for temp == 0).
 *   submit: thread-safe, returns a ticket > 0 (or -1).
 *   wait  : blocks until the request is done; copies the PCM (24 kHz mono) and returns the sample count, -1 if the generation failed,
 *           -(2 + samples) if `capacity` is too small (the ticket stays valid).  A ticket is consumed by a successful or failed wait.
 *   free  : serves what is pending, then stops the worker.  No thread may still be inside submit / wait of this batcher; tickets that were
 *           never waited for are dropped. */
struct bark_hip_batcher;
BARK_API struct bark_hip_batcher * bark_hip_batcher_create(struct bark_context * bctx, int max_batch, int max_wait_ms);
/* n_streams (1 .. 4) job streams: workers 1 .. n_streams-1 run on clones of `bctx` (bark_hip_clone_context; owned by the batcher) and serve the
 * same queue, so up to n_streams jobs are in flight on the GPU at once - two decode chains share the chip (two streams of 64-slot jobs:
 * +14 % prompts/s under load).  Results do not depend on the stream a request travelled in. */
BARK_API struct bark_hip_batcher * bark_hip_batcher_create_ex(struct bark_context * bctx, int max_batch, int max_wait_ms, int n_streams);
// One process, several GPUs.  bark_load_model (bark.h / bark.cpp:1165) takes the device from BARK_HIP_DEVICE or the current device; this variant takes it as an
// argument.  bark_hip_batcher_create_multi: a request collector whose workers are the caller's contexts - one per GPU - behind one queue (request-level
// data parallelism: no collective inside an utterance; the reference's server holds one context behind one mutex, examples/server/server.cpp:76-94).  The
// collector does not own the contexts; request defaults come from ctxs[0].  nullptr on a bad argument (null / repeated context, n_ctx outside 1 .. 64).
BARK_API struct bark_context * bark_hip_load_model_on_device(const char * model_path, struct bark_context_params params, uint32_t seed, int device);
BARK_API struct bark_hip_batcher * bark_hip_batcher_create_multi(struct bark_context * const * ctxs, int n_ctx, int max_batch, int max_wait_ms);
BARK_API int64_t bark_hip_batcher_submit(struct bark_hip_batcher * b, const char * text, uint32_t seed);
/* a request with its own parameters (nullptr: the context's) */
BARK_API int64_t bark_hip_batcher_submit_ex(struct bark_hip_batcher * b, const char * text, const struct bark_hip_request_params * params);
/* ... and its own top-k / nucleus filter; -1 for an invalid filter.  filter == nullptr: the context's filter as it was when the collector was
 * created (bark_hip_batcher_create* copy it once; a later bark_hip_set_sampling_filter on that context does not reach the collector).
 * params == nullptr: the context's parameters with seed 0, as bark_hip_batcher_submit_ex. */
BARK_API int64_t bark_hip_batcher_submit_filtered(struct bark_hip_batcher * b, const char * text, const struct bark_hip_request_params * params,
                                                  const struct bark_hip_sampling_filter * filter);
/* ... and its own voice prompt (the arrays are copied into the request); -1 for a voice bark_hip_set_voice_prompt would refuse.  voice == nullptr: the
 * context's voice as it was when the collector was created. */
BARK_API int64_t bark_hip_batcher_submit_voiced(struct bark_hip_batcher * b, const char * text, const struct bark_hip_request_params * params,
                                                const struct bark_hip_sampling_filter * filter, const struct bark_hip_voice_prompt * voice);
BARK_API int bark_hip_batcher_wait(struct bark_hip_batcher * b, int64_t ticket, float * pcm, int capacity);
/* A request whose answer comes in another rate / format (bark_hip_audio_format; -1 for an unsupported one).  The worker thread owns the context, so the
 * conversion happens there, behind the job: one bark_hip_resample_many per distinct format among the job's requests.  fmt == NULL or {24000, F32}: the
 * path of bark_hip_batcher_submit_voiced - no further launch, the same bits.  bark_hip_batcher_wait_bytes: as bark_hip_batcher_wait, in bytes of the
 * request's format (any request, f32 ones included): the byte count, -1, or -(2 + bytes) with the ticket still valid.  bark_hip_batcher_wait on a ticket
 * whose format is not {24000, F32} returns -1 and leaves the ticket valid. */
BARK_API int64_t bark_hip_batcher_submit_as(struct bark_hip_batcher * b, const char * text, const struct bark_hip_request_params * params,
                                            const struct bark_hip_sampling_filter * filter, const struct bark_hip_voice_prompt * voice,
                                            const struct bark_hip_audio_format * fmt);
BARK_API int bark_hip_batcher_wait_bytes(struct bark_hip_batcher * b, int64_t ticket, void * out, int capacity_bytes);
/* A long text as ONE ticket (bark_hip_generate_long's rules C15s / C15j; NULL pointers take its defaults, params == NULL: the context's with seed 0).
 * Only long_params->chain == 0 is accepted.  The text is split at submit time and its parts enter the queue as ordinary requests - part i with seed
 * params->seed + i - so they share jobs with other traffic and continuous admission applies; the worker that finishes the ticket's last part joins the
 * parts' audio on its own context, at fmt's rate and format.  bark_hip_batcher_wait_bytes (or bark_hip_batcher_wait for {24000, F32}) returns the joined
 * audio: what bark_hip_generate_long + bark_hip_long_audio_as give on a fresh context with the same arguments.  If a part fails, the ticket fails.
 * Returns the ticket, or -1: chain != 0, bad join parameters, a refusal of the splitter, an unsupported format, a bad filter or voice.
 * Cost on the CALLER's thread: the splitter runs here, before the call returns.  It counts every candidate span with the tokenizer itself (std::regex) and
 * is quadratic in the words of a chunk: well under a millisecond for a sentence, milliseconds for a paragraph, up to seconds for 64 chunks of 250 word
 * pieces each.  Call it from the thread that serves the request (as bark_batch_server does), never from an accept loop.
 * bark_hip_batcher_ticket_chunks: the number of parts a ticket stands for (1 for an ordinary request) while the ticket is valid, else -1. */
BARK_API int64_t bark_hip_batcher_submit_long(struct bark_hip_batcher * b, const char * text, const struct bark_hip_long_params * long_params,
                                              const struct bark_hip_request_params * params, const struct bark_hip_sampling_filter * filter,
                                              const struct bark_hip_voice_prompt * voice, const struct bark_hip_audio_format * fmt);
BARK_API int bark_hip_batcher_ticket_chunks(struct bark_hip_batcher * b, int64_t ticket);
/* bark_hip_batcher_submit_as / _submit_long with a speaking rate (rule C16t; -1 for a speed outside 500 .. 2000).  The worker runs ONE tempo launch per job
 * over all its requests with a speed other than 1000, then one bark_hip_resample_many per distinct format as before; a long text's parts are time-scaled in
 * one launch in front of its join.  speed_permille == 1000: the path of the form without a speed.  bark_hip_batcher_wait_bytes returns the result
 * (bark_hip_batcher_wait too where the format is {24000, F32}). */
BARK_API int64_t bark_hip_batcher_submit_at(struct bark_hip_batcher * b, const char * text, const struct bark_hip_request_params * params,
                                            const struct bark_hip_sampling_filter * filter, const struct bark_hip_voice_prompt * voice,
                                            const struct bark_hip_audio_format * fmt, int speed_permille);
BARK_API int64_t bark_hip_batcher_submit_long_at(struct bark_hip_batcher * b, const char * text, const struct bark_hip_long_params * long_params,
                                                 const struct bark_hip_request_params * params, const struct bark_hip_sampling_filter * filter,
                                                 const struct bark_hip_voice_prompt * voice, const struct bark_hip_audio_format * fmt, int speed_permille);
/* bark_hip_batcher_submit_at / _submit_long_at with a levelling too (rule C17l; `how` as for bark_hip_get_audio_with, -1 for what that call refuses).  The
 * worker runs ONE measure launch and ONE level launch per job over all its requests with levelling on, in front of the single tempo launch; a long text's parts
 * are levelled, each on its own, in front of tempo and join.  Levelling off: the path of the _at form. */
BARK_API int64_t bark_hip_batcher_submit_with(struct bark_hip_batcher * b, const char * text, const struct bark_hip_request_params * params,
                                              const struct bark_hip_sampling_filter * filter, const struct bark_hip_voice_prompt * voice,
                                              const struct bark_hip_audio_render * how);
BARK_API int64_t bark_hip_batcher_submit_long_with(struct bark_hip_batcher * b, const char * text, const struct bark_hip_long_params * long_params,
                                                   const struct bark_hip_request_params * params, const struct bark_hip_sampling_filter * filter,
                                                   const struct bark_hip_voice_prompt * voice, const struct bark_hip_audio_render * how);
BARK_API void bark_hip_batcher_stats(struct bark_hip_batcher * b, int * n_batches, int * n_requests, int * largest_batch);
/* requests that joined a job that was already running (continuous admission: while the semantic stage of a job has free slots, requests
 * arriving in the meantime are taken along, up to max_batch per job) */
BARK_API int bark_hip_batcher_admitted(struct bark_hip_batcher * b);
BARK_API void bark_hip_batcher_free(struct bark_hip_batcher * b);

/* Token streams of the last bark_generate_audio call (copied out; returns counts). */
BARK_API int bark_hip_get_semantic_tokens(struct bark_context * bctx, int32_t * out, int capacity);
BARK_API int bark_hip_get_coarse_tokens(struct bark_context * bctx, int32_t * out_Tx2, int capacity_rows);
BARK_API int bark_hip_get_fine_tokens(struct bark_context * bctx, int32_t * out_Tx8, int capacity_rows);

/* Detailed statistics of the last bark_generate_audio call. */
struct bark_hip_stats {
    int64_t t_load_us, t_eval_us;
    int64_t t_semantic_us, t_coarse_us, t_fine_us, t_codec_us;   /* host wall clock per stage        */
    int64_t n_sample_semantic, n_sample_coarse, n_sample_fine;   /* same quotient as bark.cpp:176-182 */
    int32_t n_semantic, n_frames, n_samples;
    int32_t n_near_tie;                                          /* greedy picks settled on the host  */
    int32_t graph_replays;                                       /* hipGraph launches issued          */
    int32_t n_prefix_rows_reused;                                /* coarse prompt rows served from the KV cache */
};
BARK_API void bark_hip_get_stats(struct bark_context * bctx, struct bark_hip_stats * out);

/* Micro-benchmark hook used by bench.py for the roofline line: runs `iters` decode steps of model
 * `which` at context length `ctx` on the context's stream and returns the average device time of
 * one step in microseconds (hipEvents on that stream); *bytes_per_step receives the algorithmic
 * bytes of one step (weights + KV rows read).  Returns <0 on error. */
BARK_API double bark_hip_time_decode_step(struct bark_context * bctx, int which, int ctx, int iters,
                                          double * bytes_per_step);

/* Device time (us) of ONE decode GEMV kernel launch (gemv_kernel), averaged over `iters` back-to-back launches that
 * rotate through the layers' weights.  op: 0 LN+QKV, 1 attention out-proj, 2 LN+FC+GELU, 3 MLP out-proj.
 * *bytes_per_launch receives the algorithmic bytes (the weight matrix in the file's format: f16, f32 or blocks). */
BARK_API double bark_hip_time_gemv(struct bark_context * bctx, int which, int op, int iters, double * bytes_per_launch);

/* Device time (us) of ONE lock-step decode kernel over n_slots utterance slots (the kernels of bark_hip_generate_batch), averaged over
 * `iters` back-to-back launches that rotate through the layers' weights.  op: 0 QKV, 1 attention out-proj, 2 FC + GELU, 3 MLP out-proj,
 * 4 LayerNorm of the slot rows, 5 attention of every slot at context `ctx`.  kind: 0 = the VALU GEMV per pair of slots with the LayerNorm fused
 * (ops 0 / 2) and, for op 5, one workgroup per (head, slot); 6 = the matrix-core product with the LayerNorm fused (ops 0 / 2); any other value =
 * the matrix-core product on normalised f16 rows and, for op 5, the scores + mix pair of launches where the engine would use it.  f16 model files, and
 * f32 model files with kind 0 for ops 0 - 3 (the slot-group product gemv_w32_slots_kernel) and op 5; an f32 file has no op 4 and no matrix-core kinds, a
 * block-quantised file none of this (< 0). */
BARK_API double bark_hip_time_slots(struct bark_context * bctx, int which, int op, int n_slots, int kind, int ctx, int iters);

/* Time line of ONE lock step over n_slots slots of model `which` (0 semantic, 1 coarse) at context `ctx`: the step is enqueued eagerly `reps`
 * times with a HIP event behind every launch site; writes a JSON array [{"site": ..., "us": average time from the previous event}, ...] in
 * launch order (kernel time + the gap in front of it), closed by {"site": "step (graph replay)", "us": the same step replayed from its
 * hipGraph}.  Returns the length written, or -1 (error / capacity too small). */
BARK_API int bark_hip_profile_lock_step(struct bark_context * bctx, int which, int n_slots, int ctx, int reps, char * json_out, int capacity);

/* Kernel-level hook of the semantic / coarse sampler with the top-k / nucleus filter (tests): n_rows rows of n logits (n <= 12288), row r sampled with
 * temp[r] (> 0), top_k[r], top_p[r] and the uniform draw u[r] by the decode loop's launches (filter, then the multinomial sampler of C8) on the
 * context's stream.  out_ids[r]: the pick, out_eos_p[r]: the probability of the last id (0 if the filter removed it).  Returns 0, or -1. */
BARK_API int bark_hip_sample_rows_filtered(struct bark_context * bctx, const float * logits, int n_rows, int n, const float * temp, const int32_t * top_k,
                                           const float * top_p, const double * u, int32_t * out_ids, float * out_eos_p);
/* Kernel-level hook that reaches the whole semantic / coarse sampler (tests): as bark_hip_sample_rows_filtered, with temp[r] >= 0 (0: the greedy
 * pick), a stop threshold min_eos_p[r] per row, the row's stage state before the launch and the per-call settings below.  state_io holds eight
 * int32 per row in the order n_past, cur_token, step, eos_step, near_tie, n_out, last_eos_p (float bits), fault: the state before the launch on
 * entry (step and n_out in 0..7, n_past in 0..2^30), the state after it on return.  near_tie counts the samples settled by the exact path.
 * out_ids[r]: the id the launch stored, out_eos_p[r]: the probability of the last id (mode 1: the state's last_eos_p).  Returns 0, or -1. */
struct bark_hip_sample_call {
    int32_t mode;          /* 0 semantic (stop rule), 1 coarse (id = pick + token_base + 1024 * (step & 1), no stop rule) */
    int32_t eos_token;     /* mode 0: a pick of this id stops (-1: none) */
    int32_t token_base;    /* mode 1: start of the coarse ids, 0..2^30 */
    int32_t prescaled;     /* 1: greedy rows hold logits already divided by 0.7 (the decode step's LM head), 0: raw logits */
    int32_t n_past_add;    /* added to the state's n_past, 0..1024 */
    int32_t per_row;       /* 1: one launch per row in the form of bark_generate_audio (one slot, scalar temp / min_eos_p), at most 256 rows;
                              0: the rows are the slots of lock-step launches (per-slot arrays, chunks of up to 4096 rows) */
};
BARK_API int bark_hip_sample_rows_state(struct bark_context * bctx, const float * logits, int n_rows, int n, const float * temp, const int32_t * top_k,
                                        const float * top_p, const double * u, const float * min_eos_p, const struct bark_hip_sample_call * call,
                                        int32_t * state_io, int32_t * out_ids, float * out_eos_p);
/* Device time (us) of ONE filter launch over n_slots rows of n logits (the filter kernel alone, averaged over `iters` launches on rows that are
 * restored in between); peaked != 0: logits with a nucleus of a few hundred ids, 0: nearly flat logits.  Returns < 0 on error. */
BARK_API double bark_hip_time_sample_filter(struct bark_context * bctx, int n, int n_slots, int32_t top_k, float top_p, int peaked, int iters);

/* Device time (us) of one fine forward pass (N = 1024), averaged over iters. */
BARK_API double bark_hip_time_fine_pass(struct bark_context * bctx, int iters, double * flops_per_pass);
/* the same for n_windows fine windows side by side (the forward pass of bark_hip_fine_many / of a lock-step batch); flops for all windows */
BARK_API double bark_hip_time_fine_passes(struct bark_context * bctx, int n_windows, int iters, double * flops_per_pass);

/* Library / device description (static string). */
// Order of the fine model's weight products on f16 model files (bark.cpp:1489,1533,1552,1558,1573: ggml_mul_mat of the fine graph).
//   0  default policy: C1 (the restated reference order; f32 matrix cores) for bark_generate_audio and the stage-level entry points - greedy fine ids are
//      bit-equal to the CPU restatement of the reference - and C1m (the f16 matrix cores' own accumulation, >= 98 % of the ids equal, logits within 2.5e-3)
//      inside lock-step jobs (bark_hip_generate_batch*, the request collector) and bark_hip_fine_many;
//   1  C1 everywhere;   2  C1m everywhere (the behaviour of rounds 4 - 5).     Environment: BARK_HIP_FINE_ORDER=c1|c1m at load.  Returns 0, -1 on a bad argument.
BARK_API int bark_hip_set_fine_order(struct bark_context * bctx, int order);
BARK_API const char * bark_hip_describe(struct bark_context * bctx);

#ifdef __cplusplus
}
#endif
