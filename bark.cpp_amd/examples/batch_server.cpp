// batch_server.cpp - an HTTP front end for the MI355X Bark engine that BATCHES.
//
// Same protocol as the reference's example server (examples/server/server.cpp:128-163): POST /bark with a JSON body {"text": "..."}
// answers with a 24 kHz mono 32-bit float WAV (examples/common.cpp:11-25).  The reference serialises its requests on a mutex around
// bark_generate_audio; here every connection is a thread that hands its text to the request collector of bark_mi355x.h
// (bark_hip_batcher_*): whatever is pending travels through the engine as ONE lock-step batch.  A request may carry "seed": n (default:
// a counter starting at the server's --seed); its audio is what a fresh context loaded with that seed generates, whatever batch it joined.
// "top_k": k (integer >= 0, 0 off) and "top_p": p (0 < p <= 1, 1 off) filter the request's semantic and coarse samples (bark_hip_sampling_filter);
// a field left out takes the server's --top-k / --top-p, an invalid one is answered 400.
// "voice": "name" gives the request the voice prompt (speaker history, bark_hip_voice_prompt) loaded with --voice name=file (repeatable; the file format
// of bark.cpp_amd/voice.py); an unknown name is answered 400, a request without the field has no voice.
// Voices from a recording (--semantic-encoder file loads HuBERT and its token head, bark_hip_load_semantic_encoder; the model file must carry the codec
// encoder): --voice-audio name=file.wav at start-up, and while the server runs
//   POST /voices?name=NAME   body: a mono 24 kHz WAV (16-bit PCM or 32-bit float, at most 4 MiB) -> 200 {"name": ..., "n_semantic": ..., "n_frames": ...};
//                            400 a bad name, a bad WAV, another rate, a recording the engine refuses; 409 no semantic or codec encoder; 413 too large.
//                            An existing name is replaced; a request in flight keeps the voice it started with.
//   GET /voices              {"voices": ["NAME", ...]}
//   GET /voices/NAME         the voice as a voice prompt file (what --voice name=file reads)
// The recording is encoded by bark_hip_voice_from_audio on a clone kept for that purpose behind its own mutex: the contexts the collector owns are never
// touched by a connection thread.
// Output rate and sample format (bark_hip_audio_format, rule C14r): "sample_rate": 8000 | 12000 | 16000 | 22050 | 24000 | 32000 | 44100 | 48000 and "format": "f32" |
// "s16" | "mulaw" | "flac" in a /bark request (defaults: --sample-rate / --format, 24000 and f32) - the answer is a WAV with the matching header (IEEE float; 16-bit PCM;
// 8-bit mu-law with a fact chunk), an unsupported value is answered 400.  POST /voices?name=NAME&resample=1 (for --voice-audio: --voice-audio-resample) takes a
// recording at any of those rates and brings it to 24 kHz with bark_hip_resample on the encoder's clone; without the switch another rate stays a 400.
// Long texts (rules C15s / C15j of bark_mi355x.h): "long": true in a /bark request (default: --long) takes a text of any length - it is split into chunks
// ("max_tokens": 0 one sentence per chunk, 1 .. 255 greedy merging; default --max-tokens), the chunks travel through the collector as ordinary requests
// (chunk i with seed + i) and their audio is joined on the device with "gap_ms" of silence between them (default --gap-ms, 250) at the request's
// "sample_rate" / "format"; the answer carries X-Bark-Chunks: n.  More than 64 chunks or a malformed field is a 400.  Without "long" and --long a request
// is served as before.
// Speaking rate (rule C16t of bark_mi355x.h): "speed": a number in 0.5 .. 2.0 in a /bark request (default: --speed, 1.0), sent to the collector as
// lround(1000 speed) per mille - the answer is time-scaled on the device before "sample_rate" / "format" apply (with "long": every chunk, before the join),
// and the WAV header follows the actual sample count.  Anything else is a 400.
// FLAC (rule C18f of bark_mi355x.h): "format": "flac" (or --format flac) - the answer is a complete FLAC stream over the s16 samples, encoded on the device, with
// Content-Type: audio/flac instead of a WAV; it combines with "sample_rate", "speed", "loudness" and "long" (one stream over the joined audio).
// Loudness (rule C17l of bark_mi355x.h): "loudness": a number in -40 .. -5 (LUFS) in a /bark request (default: --loudness; off without it), sent to the
// collector as lround(100 v) hundredths with a peak ceiling of 1.0 and a gain cap of 10 (+20 dB) - the answer is levelled on the device in front of "speed",
// "sample_rate" and "format" (with "long": every chunk on its own, before the join).  Anything else is a 400 and draws no seed.
// Plain POSIX sockets, one thread per connection, Connection: close; no third-party code.
//
//   bark_batch_server -m model.bin [-a 127.0.0.1] [-p 1337] [-s seed] [--max-batch 32] [--max-wait-ms 5] [--streams 1] [--devices 0,1,...] [--temp t] [--fine-temp t] [--top-k k] [--top-p p] [--voice name=file ...] [--semantic-encoder file] [--voice-audio name=file.wav ...] [--voice-audio-resample] [--sample-rate hz] [--format f32|s16|mulaw|flac] [--long] [--max-tokens n] [--gap-ms n] [--speed x] [--loudness lufs]
#include "bark.h"
#include "bark_mi355x.h"
#include "http_util.h"

#include <arpa/inet.h>
#include <netinet/in.h>
#include <sys/socket.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <csignal>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <thread>
#include <vector>

namespace {

using barkhttp::json_string; using barkhttp::json_uint; using barkhttp::json_int; using barkhttp::json_float; using barkhttp::wav_f32;
using barkhttp::VoiceFile;

struct Options {
    std::string model, host = "127.0.0.1";
    int port = 1337, max_batch = 32, max_wait_ms = 5, streams = 1;
    std::vector<int> devices;                      // --devices 0,1,...: one context (own copy of the weights) and one worker per listed GPU, one queue
    uint32_t seed = 0;
    float temp = -1.0f, fine_temp = -1.0f;
    int32_t top_k = 0; float top_p = 1.0f;         // --top-k / --top-p: the filter of requests that carry no "top_k" / "top_p" of their own
    std::vector<std::string> voices;               // --voice name=file
    std::string semantic_encoder;                  // --semantic-encoder file
    std::vector<std::string> voice_audio;          // --voice-audio name=file.wav
    bool voice_audio_resample = false;             // --voice-audio-resample: --voice-audio recordings at any supported rate
    int sample_rate = 24000; std::string format = "f32";      // --sample-rate / --format: what a request without "sample_rate" / "format" is answered in
    bool long_form = false; int max_tokens = 0, gap_ms = 250;  // --long / --max-tokens / --gap-ms: what a request without "long" / "max_tokens" / "gap_ms" gets
    double speed = 1.0;                            // --speed: the speaking rate of a request without "speed"
    bool has_loudness = false; double loudness = 0.0;      // --loudness: the target of a request without "loudness" (none: no levelling)
};

bool send_all(int fd, const char * p, size_t n) {
    while (n) {
        const ssize_t k = ::send(fd, p, n, MSG_NOSIGNAL);
        if (k <= 0) return false;
        p += k; n -= (size_t) k;
    }
    return true;
}

// extra: further header lines, each closed by \r\n (X-Bark-Chunks of a long answer)
void respond(int fd, int status, const char * reason, const char * type, const std::string & body, const char * extra = "") {
    char head[320];
    const int n = snprintf(head, sizeof(head), "HTTP/1.1 %d %s\r\nContent-Type: %s\r\nContent-Length: %zu\r\n%sConnection: close\r\n\r\n", status, reason, type, body.size(), extra);
    if (send_all(fd, head, (size_t) n)) send_all(fd, body.data(), body.size());
}

std::atomic<uint32_t> next_seed{0};
bark_hip_request_params request_defaults{};            // the context's sampling parameters (a request with its own filter carries them explicitly)
bark_hip_sampling_filter filter_defaults{0, 1.0f};
bark_hip_audio_format format_defaults{24000, BARK_HIP_SAMPLE_F32};
// long texts (rules C15s / C15j): the route is taken by requests with "long": true (or by all of them under --long); the splitter's budget and the gap
struct LongDefaults { bool on = false; int32_t max_tokens = 0, gap_ms = 250; } long_defaults;
constexpr int kMaxGapMs = 60000;
bool long_valid(int32_t max_tokens, int32_t gap_ms) { return max_tokens >= 0 && max_tokens <= 255 && gap_ms >= 0 && gap_ms <= kMaxGapMs; }
// speaking rate (rule C16t): a factor in 0.5 .. 2.0, sent as lround(1000 speed); anything else (a NaN too) is refused
double speed_default = 1.0;
bool speed_valid(double speed) { return speed >= 0.5 && speed <= 2.0; }
int speed_permille(double speed) { return (int) lround(1000.0 * speed); }
// loudness (rule C17l): a target in -40 .. -5 LUFS, sent as lround(100 v); ceiling 1.0, cap 10 (+20 dB); anything else (a NaN too) is refused
bool loudness_default_on = false;
double loudness_default = 0.0;
bool loudness_valid(double v) { return v >= -40.0 && v <= -5.0; }
bark_hip_loudness_params loudness_request(double v) { return bark_hip_loudness_params{(int32_t) lround(100.0 * v), 1.0f, 10.0f}; }
// the body of an answer of nb bytes in the request's format: the stream itself for FLAC (rule C18f), else a WAV around the nb / width samples
std::string answer_body(const std::vector<char> & bytes, int nb, const bark_hip_audio_format & af) {
    if (af.sample_format == BARK_HIP_SAMPLE_FLAC) return std::string(bytes.data(), (size_t) nb);
    const int width = af.sample_format == BARK_HIP_SAMPLE_F32 ? 4 : af.sample_format == BARK_HIP_SAMPLE_S16 ? 2 : 1;
    return barkhttp::wav_samples(bytes.data(), nb / width, af.sample_rate, af.sample_format);
}
bool format_valid(const bark_hip_audio_format & f) { return f.sample_format >= 0 && f.sample_format <= 3 && bark_hip_resample_out_len(1, 24000, f.sample_rate) >= 1; }
// the voices by name: read by every /bark request, written by POST /voices.  An entry is never changed, only replaced: a request that has looked its
// voice up keeps it alive through its shared_ptr while a later POST puts another one under the same name
std::shared_mutex voice_mutex;
std::map<std::string, std::shared_ptr<const VoiceFile>> voice_table;
std::shared_ptr<const VoiceFile> find_voice(const std::string & name) {
    std::shared_lock<std::shared_mutex> lock(voice_mutex);
    const auto it = voice_table.find(name);
    return it == voice_table.end() ? nullptr : it->second;
}
void put_voice(const std::string & name, VoiceFile && v) {
    auto p = std::make_shared<const VoiceFile>(std::move(v));
    std::unique_lock<std::shared_mutex> lock(voice_mutex);
    voice_table[name] = std::move(p);
}
// the context that encodes recordings (a clone made after the semantic encoder was loaded, so it shares the device copy); null: no encoder available
bark_context * encoder_ctx = nullptr;
std::mutex encoder_mutex;
constexpr size_t kMaxBody = 1u << 20, kMaxVoiceBody = 4u << 20;
// a recording at another supported rate -> 24 kHz (bark_hip_resample on the encoder's clone); false: the engine refused it
bool recording_to_24k(std::vector<float> & pcm, int rate) {
    if (pcm.size() > 0x7fffffffu) return false;
    const int n_out = bark_hip_resample_out_len((int) pcm.size(), rate, 24000);
    if (n_out < 1) return false;
    std::vector<float> out((size_t) n_out);
    std::lock_guard<std::mutex> lock(encoder_mutex);
    if (bark_hip_resample(encoder_ctx, pcm.data(), (int) pcm.size(), rate, 24000, out.data(), n_out) != n_out) return false;
    pcm.swap(out);
    return true;
}
// 24 kHz mono samples -> voice; false: the engine refused the recording (its message is on stderr)
bool voice_from_recording(const std::vector<float> & pcm, VoiceFile & out) {
    const int used = (int) std::min<size_t>(pcm.size(), BARK_HIP_VOICE_AUDIO_MAX_SAMPLES);
    const int rows = (used + 319) / 320, sem_cap = std::max(1, ((2 * used + 2) / 3 - 400) / 320 + 1);
    out.semantic.assign((size_t) sem_cap, 0); out.coarse.assign((size_t) rows * 2, 0); out.fine.assign((size_t) rows * 8, 0);
    int32_t n_sem = 0, n_frames = 0;
    std::lock_guard<std::mutex> lock(encoder_mutex);
    if (pcm.size() > 0x7fffffffu || bark_hip_voice_from_audio(encoder_ctx, pcm.data(), (int) pcm.size(), out.semantic.data(), sem_cap, out.coarse.data(), out.fine.data(), rows, &n_sem, &n_frames) != 0)
        return false;
    out.semantic.resize((size_t) n_sem); out.coarse.resize((size_t) n_frames * 2); out.fine.resize((size_t) n_frames * 8);
    return true;
}
std::atomic<int> open_connections{0};
constexpr int kMaxConnections = 512;                     // beyond that a connection is answered 503 at once

void serve(int fd, bark_hip_batcher * batcher, int sample_rate) {
    struct Guard { ~Guard() { open_connections.fetch_sub(1); } } guard;
    timeval tv{10, 0};                                       // a client that stops sending does not park this thread for ever
    setsockopt(fd, SOL_SOCKET, SO_RCVTIMEO, &tv, sizeof(tv));
    std::string req;
    char buf[4096];
    size_t head_end = std::string::npos;
    while (head_end == std::string::npos && req.size() < (1u << 20)) {
        const ssize_t k = ::recv(fd, buf, sizeof(buf), 0);
        if (k <= 0) { ::close(fd); return; }
        req.append(buf, (size_t) k);
        head_end = req.find("\r\n\r\n");
    }
    if (head_end == std::string::npos) { respond(fd, 400, "Bad Request", "text/plain", "bad request"); ::close(fd); return; }
    const std::string head = req.substr(0, head_end);
    size_t content_length = 0;
    {
        std::string lower = head;
        for (char & ch : lower) ch = (char) tolower((unsigned char) ch);
        const size_t p = lower.find("content-length:");
        if (p != std::string::npos) content_length = (size_t) strtoul(head.c_str() + p + 15, nullptr, 10);
    }
    const std::string target = head.substr(0, head.find("\r\n"));      // the request line
    const bool post_voice = target.compare(0, 13, "POST /voices ") == 0 || target.compare(0, 13, "POST /voices?") == 0;
    if (content_length > (post_voice ? kMaxVoiceBody : kMaxBody)) { respond(fd, 413, "Payload Too Large", "text/plain", "too large"); ::shutdown(fd, SHUT_RDWR); ::close(fd); return; }
    std::string body = req.substr(head_end + 4);
    while (body.size() < content_length) {
        const ssize_t k = ::recv(fd, buf, sizeof(buf), 0);
        if (k <= 0) break;
        body.append(buf, (size_t) k);
    }
    if (post_voice) {
        // checked in the order: what the server can do at all, the name, the recording
        const size_t sp = target.rfind(' ');                  // "POST /voices?name=a HTTP/1.1" -> "/voices?name=a"
        const std::string path = target.substr(5, sp != std::string::npos && sp > 5 ? sp - 5 : std::string::npos);
        std::string name, err;
        std::vector<float> pcm;
        int rate = 0;
        VoiceFile vf;
        std::string rs;
        const bool may_resample = barkhttp::query_param(path, "resample", rs) && rs == "1";
        if (!encoder_ctx) respond(fd, 409, "Conflict", "text/plain", "no semantic encoder (--semantic-encoder) or no codec encoder in the model file");
        else if (!barkhttp::query_param(path, "name", name) || !barkhttp::valid_voice_name(name)) respond(fd, 400, "Bad Request", "text/plain", "expected ?name=NAME with 1 .. 64 of [A-Za-z0-9_.-]");
        else if (body.size() != content_length || !barkhttp::parse_wav(body, pcm, rate, err)) respond(fd, 400, "Bad Request", "text/plain", err.empty() ? "incomplete body" : err);
        else if (rate != 24000 && !may_resample) respond(fd, 400, "Bad Request", "text/plain", "the recording must be sampled at 24000 Hz (or send ?resample=1)");
        else if (rate != 24000 && !recording_to_24k(pcm, rate)) respond(fd, 400, "Bad Request", "text/plain", "the rate is not one the resampler takes, or the engine refused the recording");
        else if (!voice_from_recording(pcm, vf)) respond(fd, 400, "Bad Request", "text/plain", "the engine refused the recording (too short, or samples that are not finite)");
        else {
            char js[256];
            snprintf(js, sizeof(js), "{\"name\": \"%s\", \"n_semantic\": %zu, \"n_frames\": %zu}", name.c_str(), vf.semantic.size(), vf.fine.size() / 8);
            put_voice(name, std::move(vf));
            respond(fd, 200, "OK", "application/json", js);
        }
    } else if (target.compare(0, 12, "GET /voices ") == 0 || target.compare(0, 12, "GET /voices?") == 0) {
        std::string js = "{\"voices\": [";
        {
            std::shared_lock<std::shared_mutex> lock(voice_mutex);
            bool first = true;
            for (const auto & kv : voice_table) { js += std::string(first ? "\"" : ", \"") + kv.first + "\""; first = false; }      // names from --voice may hold anything but '='
        }
        respond(fd, 200, "OK", "application/json", js + "]}");
    } else if (target.compare(0, 12, "GET /voices/") == 0) {
        const size_t e = target.find_first_of(" ?", 12);
        const std::shared_ptr<const VoiceFile> v = find_voice(target.substr(12, e == std::string::npos ? std::string::npos : e - 12));
        if (v) respond(fd, 200, "OK", "application/octet-stream", barkhttp::voice_file_bytes(*v));
        else respond(fd, 404, "Not Found", "text/plain", "no such voice");
    } else if (head.compare(0, 4, "GET ") == 0) {
        respond(fd, 200, "OK", "text/html", "<html>bark batch server: POST /bark {\"text\": \"...\"}</html>");
    } else if (head.compare(0, 11, "POST /bark ") == 0 || head.compare(0, 11, "POST /bark?") == 0) {
        std::string text;
        if (!json_string(body, "text", text)) {
            respond(fd, 400, "Bad Request", "text/plain", "expected a JSON body with a \"text\" string");
        } else {
            // "top_k" (integer >= 0) / "top_p" (0 < p <= 1): the request's own filter, the other field from the server's defaults.  Checked
            // before a default seed is drawn: a refused request does not shift the seeds of the requests behind it
            bark_hip_sampling_filter flt = filter_defaults;
            const int hk = json_int(body, "top_k", flt.top_k), hp = json_float(body, "top_p", flt.top_p);
            int64_t ticket = -1;
            if (hk < 0 || hp < 0 || flt.top_k < 0 || !(flt.top_p > 0.0f && flt.top_p <= 1.0f)) {
                respond(fd, 400, "Bad Request", "text/plain", "\"top_k\" must be an integer >= 0 and \"top_p\" a number in (0, 1]");
                ::shutdown(fd, SHUT_RDWR);
                ::close(fd);
                return;
            }
            // "sample_rate" / "format": what the answer comes in; checked here as well, for the same reason
            bark_hip_audio_format af = format_defaults;
            if (!barkhttp::request_format(body, af.sample_rate, af.sample_format) || !format_valid(af)) {
                respond(fd, 400, "Bad Request", "text/plain", "\"sample_rate\" must be 8000, 12000, 16000, 22050, 24000, 32000, 44100 or 48000 and \"format\" \"f32\", \"s16\", \"mulaw\" or \"flac\"");
                ::shutdown(fd, SHUT_RDWR);
                ::close(fd);
                return;
            }
            // "long": true / false, "max_tokens": 0 .. 255, "gap_ms": 0 .. 60000 - the long-form route; checked here as well, for the same reason
            bool is_long = long_defaults.on;
            int32_t max_tokens = long_defaults.max_tokens, gap_ms = long_defaults.gap_ms;
            const int hl = barkhttp::json_bool(body, "long", is_long), hm = json_int(body, "max_tokens", max_tokens), hg = json_int(body, "gap_ms", gap_ms);
            if (hl < 0 || hm < 0 || hg < 0 || !long_valid(max_tokens, gap_ms)) {
                respond(fd, 400, "Bad Request", "text/plain", "\"long\" must be true or false, \"max_tokens\" an integer in 0 .. 255 and \"gap_ms\" an integer in 0 .. 60000");
                ::shutdown(fd, SHUT_RDWR);
                ::close(fd);
                return;
            }
            // "speed": a number in 0.5 .. 2.0 - the speaking rate; checked here as well, for the same reason
            double speed = speed_default;
            const int hs = barkhttp::json_number(body, "speed", speed);
            if (hs < 0 || !speed_valid(speed)) {
                respond(fd, 400, "Bad Request", "text/plain", "\"speed\" must be a number in 0.5 .. 2.0");
                ::shutdown(fd, SHUT_RDWR);
                ::close(fd);
                return;
            }
            const int permille = speed_permille(speed);
            // "loudness": a number in -40 .. -5 - the target in LUFS; checked here as well, for the same reason
            double loudness = loudness_default;
            const int hu = barkhttp::json_number(body, "loudness", loudness);
            const bool levels = hu > 0 || loudness_default_on;
            if (hu < 0 || (levels && !loudness_valid(loudness))) {
                respond(fd, 400, "Bad Request", "text/plain", "\"loudness\" must be a number in -40 .. -5");
                ::shutdown(fd, SHUT_RDWR);
                ::close(fd);
                return;
            }
            const bark_hip_audio_render how{af, permille, levels ? loudness_request(loudness) : bark_hip_loudness_params{0, 0.0f, 0.0f}};
            const bool plain = af.sample_rate == 24000 && af.sample_format == BARK_HIP_SAMPLE_F32 && permille == 1000 && !levels;
            // "voice": absent - no voice; otherwise a string that names a voice of the table (held until the answer is sent)
            std::shared_ptr<const VoiceFile> vf;
            int has_voice = 0;
            {
                std::shared_lock<std::shared_mutex> lock(voice_mutex);
                has_voice = barkhttp::request_voice(body, voice_table, &vf);
            }
            if (has_voice < 0) {
                respond(fd, 400, "Bad Request", "text/plain", "\"voice\" must name a voice loaded with --voice name=file, --voice-audio or POST /voices");
                ::shutdown(fd, SHUT_RDWR);
                ::close(fd);
                return;
            }
            uint32_t seed = 0;
            if (!json_uint(body, "seed", seed)) seed = next_seed.fetch_add(1);
            if (is_long) {
                // one ticket for the whole text (bark_hip_batcher_submit_long splits on this connection's thread; chunk i runs with seed + i); the answer
                // is the joined audio in the request's rate and format, the chunk count travels in X-Bark-Chunks.  A text of more than 64 chunks is a 400
                bark_hip_request_params rp = request_defaults; rp.seed = seed;
                bark_hip_voice_prompt vp{};
                if (vf) vp = bark_hip_voice_prompt{vf->semantic.data(), (int32_t) vf->semantic.size(), vf->coarse.data(), (int32_t) (vf->coarse.size() / 2),
                                                   vf->fine.data(), (int32_t) (vf->fine.size() / 8)};
                const bark_hip_long_params lp{max_tokens, 0, {gap_ms * 24, 0, 0.0f, 0}};
                ticket = levels           ? bark_hip_batcher_submit_long_with(batcher, text.c_str(), &lp, &rp, &flt, vf ? &vp : nullptr, &how)
                       : permille == 1000 ? bark_hip_batcher_submit_long(batcher, text.c_str(), &lp, &rp, &flt, vf ? &vp : nullptr, &af)
                                          : bark_hip_batcher_submit_long_at(batcher, text.c_str(), &lp, &rp, &flt, vf ? &vp : nullptr, &af, permille);
                if (ticket <= 0) {
                    respond(fd, 400, "Bad Request", "text/plain", "the text gives more than 64 chunks");
                } else {
                    char extra[64];
                    snprintf(extra, sizeof(extra), "X-Bark-Chunks: %d\r\n", bark_hip_batcher_ticket_chunks(batcher, ticket));
                    int nb = bark_hip_batcher_wait_bytes(batcher, ticket, nullptr, 0);                 // probe: -(2 + bytes)
                    if (nb <= -2) {
                        std::vector<char> bytes((size_t) std::max(-nb - 2, 1));
                        nb = bark_hip_batcher_wait_bytes(batcher, ticket, bytes.data(), -nb - 2);
                        if (nb >= 0) respond(fd, 200, "OK", barkhttp::answer_type(af.sample_format), answer_body(bytes, nb, af), extra);
                    }
                    if (nb < 0) respond(fd, 500, "Internal Server Error", "text/plain", "Internal Server Error");
                }
                ::shutdown(fd, SHUT_RDWR);
                ::close(fd);
                return;
            }
            if (!plain) {
                bark_hip_request_params rp = request_defaults; rp.seed = seed;
                bark_hip_voice_prompt vp{};
                if (vf) vp = bark_hip_voice_prompt{vf->semantic.data(), (int32_t) vf->semantic.size(), vf->coarse.data(), (int32_t) (vf->coarse.size() / 2),
                                                   vf->fine.data(), (int32_t) (vf->fine.size() / 8)};
                ticket = levels           ? bark_hip_batcher_submit_with(batcher, text.c_str(), &rp, &flt, vf ? &vp : nullptr, &how)
                       : permille == 1000 ? bark_hip_batcher_submit_as(batcher, text.c_str(), &rp, &flt, vf ? &vp : nullptr, &af)
                                          : bark_hip_batcher_submit_at(batcher, text.c_str(), &rp, &flt, vf ? &vp : nullptr, &af, permille);
                int nb = ticket > 0 ? bark_hip_batcher_wait_bytes(batcher, ticket, nullptr, 0) : -1;     // probe: -(2 + bytes)
                if (nb <= -2) {
                    std::vector<char> bytes((size_t) (-nb - 2));
                    nb = bark_hip_batcher_wait_bytes(batcher, ticket, bytes.data(), (int) bytes.size());
                    if (nb >= 0) respond(fd, 200, "OK", barkhttp::answer_type(af.sample_format), answer_body(bytes, nb, af));
                }
                if (nb < 0) respond(fd, 500, "Internal Server Error", "text/plain", "Internal Server Error");
                ::shutdown(fd, SHUT_RDWR);
                ::close(fd);
                return;
            }
            if (vf) {
                bark_hip_request_params rp = request_defaults; rp.seed = seed;
                const bark_hip_voice_prompt vp{vf->semantic.data(), (int32_t) vf->semantic.size(), vf->coarse.data(), (int32_t) (vf->coarse.size() / 2),
                                               vf->fine.data(), (int32_t) (vf->fine.size() / 8)};
                ticket = bark_hip_batcher_submit_voiced(batcher, text.c_str(), &rp, &flt, &vp);
            } else if (hk || hp) {
                bark_hip_request_params rp = request_defaults; rp.seed = seed;
                ticket = bark_hip_batcher_submit_filtered(batcher, text.c_str(), &rp, &flt);
            } else {
                ticket = bark_hip_batcher_submit(batcher, text.c_str(), seed);
            }
            int n = ticket > 0 ? bark_hip_batcher_wait(batcher, ticket, nullptr, 0) : -1;     // probe: -(2 + samples)
            if (n <= -2) {
                std::vector<float> pcm((size_t) (-n - 2));
                n = bark_hip_batcher_wait(batcher, ticket, pcm.data(), (int) pcm.size());
                if (n >= 0) respond(fd, 200, "OK", "audio/wav", wav_f32(pcm.data(), n, sample_rate));
            }
            if (n < 0) respond(fd, 500, "Internal Server Error", "text/plain", "Internal Server Error");
        }
    } else {
        respond(fd, 404, "Not Found", "text/plain", "not found");
    }
    ::shutdown(fd, SHUT_RDWR);
    ::close(fd);
}

void usage(const char * argv0) {
    fprintf(stderr, "usage: %s -m model.bin [-a host] [-p port] [-s seed] [--max-batch n (<= 256; the context serves up to 64 at a time)] [--max-wait-ms n] [--streams n (1 .. 4 jobs in flight)] [--devices 0,1,... (one context and one worker per GPU, one queue)] [--temp t] [--fine-temp t] [--top-k k (0: off)] [--top-p p (1: off)] [--voice name=file (repeatable; a request selects one with \"voice\": \"name\")] [--semantic-encoder file (HuBERT + token head: voices from recordings)] [--voice-audio name=file.wav (repeatable; mono 24 kHz)] [--voice-audio-resample (recordings at 8000 .. 48000 Hz)] [--sample-rate hz (8000 .. 48000; a request's \"sample_rate\")] [--format f32|s16|mulaw|flac (a request's \"format\")] [--long (every request takes the long-form route; a request's \"long\")] [--max-tokens n (0: one sentence per chunk, 1 .. 255: merge up to n word pieces; a request's \"max_tokens\")] [--gap-ms n (silence between chunks, default 250; a request's \"gap_ms\")] [--speed x (speaking rate 0.5 .. 2.0, default 1; a request's \"speed\")] [--loudness lufs (target -40 .. -5, default: no levelling; a request's \"loudness\")]\n", argv0);
}

}  // namespace

int main(int argc, char ** argv) {
    Options o;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        auto next = [&](const char * what) -> const char * { if (i + 1 >= argc) { fprintf(stderr, "missing value for %s\n", what); usage(argv[0]); exit(1); } return argv[++i]; };
        if (a == "-m" || a == "--model") o.model = next("-m");
        else if (a == "-a" || a == "--address") o.host = next("-a");
        else if (a == "-p" || a == "--port") o.port = atoi(next("-p"));
        else if (a == "-s" || a == "--seed") o.seed = (uint32_t) strtoul(next("-s"), nullptr, 10);
        else if (a == "--max-batch") o.max_batch = atoi(next("--max-batch"));
        else if (a == "--max-wait-ms") o.max_wait_ms = atoi(next("--max-wait-ms"));
        else if (a == "--streams") o.streams = atoi(next("--streams"));
        else if (a == "--devices") { for (const char * p = next("--devices"); *p;) { char * e = nullptr; o.devices.push_back((int) strtol(p, &e, 10)); if (e == p) { usage(argv[0]); return 1; } p = *e == ',' ? e + 1 : e; } }
        else if (a == "--temp") o.temp = (float) atof(next("--temp"));
        else if (a == "--fine-temp") o.fine_temp = (float) atof(next("--fine-temp"));
        else if (a == "--top-k") o.top_k = (int32_t) atoi(next("--top-k"));
        else if (a == "--top-p") o.top_p = (float) atof(next("--top-p"));
        else if (a == "--voice") o.voices.push_back(next("--voice"));
        else if (a == "--semantic-encoder") o.semantic_encoder = next("--semantic-encoder");
        else if (a == "--voice-audio") o.voice_audio.push_back(next("--voice-audio"));
        else if (a == "--voice-audio-resample") o.voice_audio_resample = true;
        else if (a == "--sample-rate") o.sample_rate = atoi(next("--sample-rate"));
        else if (a == "--format") o.format = next("--format");
        else if (a == "--long") o.long_form = true;
        else if (a == "--max-tokens") o.max_tokens = atoi(next("--max-tokens"));
        else if (a == "--gap-ms") o.gap_ms = atoi(next("--gap-ms"));
        else if (a == "--speed") o.speed = atof(next("--speed"));
        else if (a == "--loudness") { o.loudness = atof(next("--loudness")); o.has_loudness = true; }
        else { usage(argv[0]); return a == "-h" || a == "--help" ? 0 : 1; }
    }
    if (o.model.empty()) { usage(argv[0]); return 1; }
    format_defaults = bark_hip_audio_format{o.sample_rate, barkhttp::sample_format_of(o.format)};
    if (!format_valid(format_defaults)) { fprintf(stderr, "%s: --sample-rate must be 8000, 12000, 16000, 22050, 24000, 32000, 44100 or 48000 and --format f32, s16, mulaw or flac\n", argv[0]); return 1; }
    long_defaults.on = o.long_form; long_defaults.max_tokens = o.max_tokens; long_defaults.gap_ms = o.gap_ms;
    if (!long_valid(o.max_tokens, o.gap_ms)) { fprintf(stderr, "%s: --max-tokens must be 0 .. 255 and --gap-ms 0 .. 60000\n", argv[0]); return 1; }
    speed_default = o.speed;
    if (!speed_valid(o.speed)) { fprintf(stderr, "%s: --speed must be 0.5 .. 2.0\n", argv[0]); return 1; }
    loudness_default_on = o.has_loudness; loudness_default = o.loudness;
    if (o.has_loudness && !loudness_valid(o.loudness)) { fprintf(stderr, "%s: --loudness must be -40 .. -5\n", argv[0]); return 1; }
    {
        std::map<std::string, VoiceFile> files;
        for (const std::string & v : o.voices) {
            std::string err;
            if (!barkhttp::add_voice(files, v, err)) { fprintf(stderr, "%s: %s\n", argv[0], err.c_str()); return 1; }
        }
        for (auto & kv : files) put_voice(kv.first, std::move(kv.second));
    }
    signal(SIGPIPE, SIG_IGN);
    bark_context_params params = bark_context_default_params();
    if (o.temp >= 0.0f) params.temp = o.temp;
    if (o.fine_temp >= 0.0f) params.fine_temp = o.fine_temp;
    // one GPU: the context of bark_load_model (+ --streams job streams on clones of it); --devices: a context per listed GPU behind one queue
    std::vector<bark_context *> ctxs;
    if (o.devices.empty()) ctxs.push_back(bark_load_model(o.model.c_str(), params, o.seed));
    else for (int d : o.devices) ctxs.push_back(bark_hip_load_model_on_device(o.model.c_str(), params, o.seed, d));
    for (bark_context * c : ctxs) if (!c) { fprintf(stderr, "%s: could not load the model\n", argv[0]); for (bark_context * x : ctxs) if (x) bark_free(x); return 1; }
    for (bark_context * c : ctxs)
        if (bark_hip_set_sampling_filter(c, o.top_k, o.top_p) != 0) { fprintf(stderr, "%s: --top-k must be >= 0 and --top-p in (0, 1]\n", argv[0]); for (bark_context * x : ctxs) bark_free(x); return 1; }
    filter_defaults = bark_hip_sampling_filter{o.top_k, o.top_p};
    request_defaults.temp = params.temp; request_defaults.fine_temp = params.fine_temp; request_defaults.min_eos_p = params.min_eos_p;
    request_defaults.n_steps_text_encoder = params.n_steps_text_encoder;
    // a voice the engine would refuse (ids out of range, empty trimmed history, too long for the coarse context) is refused here, not at the first
    // request that names it; the contexts themselves keep no voice: a request without the field has none
    for (const auto & kv : voice_table) {
        const VoiceFile & vf = *kv.second;
        const bark_hip_voice_prompt vp{vf.semantic.data(), (int32_t) vf.semantic.size(), vf.coarse.data(), (int32_t) (vf.coarse.size() / 2), vf.fine.data(), (int32_t) (vf.fine.size() / 8)};
        if (bark_hip_set_voice_prompt(ctxs[0], &vp) != 0) { fprintf(stderr, "%s: voice '%s' was refused\n", argv[0], kv.first.c_str()); for (bark_context * x : ctxs) bark_free(x); return 1; }
    }
    (void) bark_hip_set_voice_prompt(ctxs[0], nullptr);
    bark_context * ctx = ctxs[0];
    // the semantic encoder goes into context 0 BEFORE any clone is made: the clones made afterwards (the encoder's below, the collector's streams) share
    // the device copy.  One further clone encodes recordings; the collector owns the others
    auto fail = [&](const std::string & why) { fprintf(stderr, "%s: %s\n", argv[0], why.c_str()); if (encoder_ctx) bark_free(encoder_ctx); for (bark_context * x : ctxs) bark_free(x); return 1; };
    if (!o.semantic_encoder.empty() && bark_hip_load_semantic_encoder(ctx, o.semantic_encoder.c_str()) != 0) return fail("could not load the semantic encoder " + o.semantic_encoder);
    if (bark_hip_has_semantic_encoder(ctx) && bark_hip_has_codec_encoder(ctx)) {
        encoder_ctx = bark_hip_clone_context(ctx, o.seed);
        if (!encoder_ctx) return fail("could not clone a context for the encoders");
    }
    for (const std::string & arg : o.voice_audio) {
        const size_t eq = arg.find('=');
        if (eq == std::string::npos || eq + 1 >= arg.size() || !barkhttp::valid_voice_name(arg.substr(0, eq))) return fail("--voice-audio expects name=file.wav, the name 1 .. 64 of [A-Za-z0-9_.-]");
        if (!encoder_ctx) return fail("--voice-audio needs --semantic-encoder and a model file with the codec encoder");
        std::string body, err;
        std::vector<float> pcm;
        int rate = 0;
        VoiceFile vf;
        FILE * f = fopen(arg.substr(eq + 1).c_str(), "rb");
        if (!f) return fail("cannot open " + arg.substr(eq + 1));
        char buf[65536];
        for (size_t k; body.size() <= kMaxVoiceBody && (k = fread(buf, 1, sizeof(buf), f)) > 0;) body.append(buf, k);
        fclose(f);
        if (body.size() > kMaxVoiceBody) return fail(arg.substr(eq + 1) + ": larger than 4 MiB");
        if (!barkhttp::parse_wav(body, pcm, rate, err)) return fail(arg.substr(eq + 1) + ": " + err);
        if (rate != 24000 && !o.voice_audio_resample) return fail(arg.substr(eq + 1) + ": the recording must be sampled at 24000 Hz (or pass --voice-audio-resample)");
        if (rate != 24000 && !recording_to_24k(pcm, rate)) return fail(arg.substr(eq + 1) + ": the rate is not one the resampler takes, or the engine refused the recording");
        if (!voice_from_recording(pcm, vf)) return fail(arg.substr(eq + 1) + ": the engine refused the recording");
        put_voice(arg.substr(0, eq), std::move(vf));
    }
    bark_hip_batcher * batcher = ctxs.size() > 1 ? bark_hip_batcher_create_multi(ctxs.data(), (int) ctxs.size(), o.max_batch, o.max_wait_ms)
                                                 : bark_hip_batcher_create_ex(ctx, o.max_batch, o.max_wait_ms, o.streams);
    if (!batcher) { fprintf(stderr, "%s: could not create the request collector\n", argv[0]); for (bark_context * x : ctxs) bark_free(x); return 1; }
    next_seed = o.seed;

    const int lfd = ::socket(AF_INET, SOCK_STREAM, 0);
    int one = 1;
    setsockopt(lfd, SOL_SOCKET, SO_REUSEADDR, &one, sizeof(one));
    sockaddr_in addr{};
    addr.sin_family = AF_INET; addr.sin_port = htons((uint16_t) o.port);
    if (inet_pton(AF_INET, o.host.c_str(), &addr.sin_addr) != 1 || bind(lfd, reinterpret_cast<sockaddr *>(&addr), sizeof(addr)) != 0 || listen(lfd, 128) != 0) {
        fprintf(stderr, "couldn't bind to server socket: hostname=%s port=%d\n", o.host.c_str(), o.port);
        bark_hip_batcher_free(batcher); for (bark_context * x : ctxs) bark_free(x);
        return 1;
    }
    printf("\nbark batch server listening at http://%s:%d (lock-step batches of up to %d requests, %d ms to fill)\n\n", o.host.c_str(), o.port, o.max_batch, o.max_wait_ms);
    fflush(stdout);
    while (true) {
        const int fd = ::accept(lfd, nullptr, nullptr);
        if (fd < 0) continue;
        if (open_connections.fetch_add(1) >= kMaxConnections) {
            open_connections.fetch_sub(1);
            respond(fd, 503, "Service Unavailable", "text/plain", "too many connections");
            ::close(fd);
            continue;
        }
        std::thread(serve, fd, batcher, params.sample_rate).detach();
    }
}
