// http_util.h - the request-side helpers of batch_server.cpp (flat-JSON field access, 32-bit float WAV framing, WAV parsing, voice prompt files), header-only
// so that a CPU test can drive them without a device (tests/test_host_frontend.py, tests/test_voice_audio_frontend.py).
#pragma once
#include <cctype>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

namespace barkhttp {

// the string value of `key` in a flat JSON object (escapes \" \\ \/ \n \t \r \b \f and \uXXXX incl. surrogate pairs are decoded to UTF-8)
inline bool json_string(const std::string & js, const char * key, std::string & out) {
    const std::string pat = std::string("\"") + key + "\"";
    size_t p = js.find(pat);
    if (p == std::string::npos) return false;
    p = js.find(':', p + pat.size());
    if (p == std::string::npos) return false;
    p++;
    while (p < js.size() && (js[p] == ' ' || js[p] == '\t' || js[p] == '\n' || js[p] == '\r')) p++;
    if (p >= js.size() || js[p] != '"') return false;            // the value of `key` must itself be a string ({"text": 12, "x": "y"} has no text)
    out.clear();
    for (size_t i = p + 1; i < js.size(); i++) {
        const char ch = js[i];
        if (ch == '"') return true;
        if (ch != '\\') { out.push_back(ch); continue; }
        if (++i >= js.size()) return false;
        switch (js[i]) {
            case 'n': out.push_back('\n'); break;
            case 't': out.push_back('\t'); break;
            case 'r': out.push_back('\r'); break;
            case 'b': out.push_back('\b'); break;
            case 'f': out.push_back('\f'); break;
            case 'u': {
                if (i + 4 >= js.size()) return false;
                unsigned cp = (unsigned) strtoul(js.substr(i + 1, 4).c_str(), nullptr, 16);
                i += 4;
                if (cp >= 0xD800 && cp < 0xDC00 && i + 6 < js.size() && js[i + 1] == '\\' && js[i + 2] == 'u') {      // surrogate pair -> one code point
                    const unsigned lo = (unsigned) strtoul(js.substr(i + 3, 4).c_str(), nullptr, 16);
                    if (lo >= 0xDC00 && lo < 0xE000) { cp = 0x10000 + ((cp - 0xD800) << 10) + (lo - 0xDC00); i += 6; }
                }
                if (cp >= 0x10000) {
                    out.push_back((char) (0xF0 | (cp >> 18))); out.push_back((char) (0x80 | ((cp >> 12) & 0x3F)));
                    out.push_back((char) (0x80 | ((cp >> 6) & 0x3F))); out.push_back((char) (0x80 | (cp & 0x3F)));
                }
                else if (cp < 0x80) out.push_back((char) cp);
                else if (cp < 0x800) { out.push_back((char) (0xC0 | (cp >> 6))); out.push_back((char) (0x80 | (cp & 0x3F))); }
                else { out.push_back((char) (0xE0 | (cp >> 12))); out.push_back((char) (0x80 | ((cp >> 6) & 0x3F))); out.push_back((char) (0x80 | (cp & 0x3F))); }
                break;
            }
            default: out.push_back(js[i]); break;            // \" \\ \/
        }
    }
    return false;
}
inline bool json_uint(const std::string & js, const char * key, uint32_t & out) {
    const std::string pat = std::string("\"") + key + "\"";
    size_t p = js.find(pat);
    if (p == std::string::npos) return false;
    p = js.find(':', p + pat.size());
    if (p == std::string::npos) return false;
    p++;
    while (p < js.size() && (js[p] == ' ' || js[p] == '\t')) p++;
    if (p >= js.size() || js[p] < '0' || js[p] > '9') return false;
    out = (uint32_t) strtoul(js.c_str() + p, nullptr, 10);
    return true;
}

// the value of `key` as a boolean (the literals true / false): 0 the key is absent, 1 *out holds it, -1 the key is there with another value
inline int json_bool(const std::string & js, const char * key, bool & out) {
    const std::string pat = std::string("\"") + key + "\"";
    size_t p = js.find(pat);
    if (p == std::string::npos) return 0;
    p = js.find(':', p + pat.size());
    if (p == std::string::npos) return -1;
    p++;
    while (p < js.size() && (js[p] == ' ' || js[p] == '\t')) p++;
    const bool t = js.compare(p, 4, "true") == 0, f = js.compare(p, 5, "false") == 0;
    if (!t && !f) return -1;
    const size_t e = p + (t ? 4 : 5);
    if (e < js.size() && (isalnum((unsigned char) js[e]) || js[e] == '_')) return -1;
    out = t;
    return 1;
}

// the value of `key` as a number: 0 the key is absent, 1 *out holds it, -1 the key is there but its value is not a number (a server answers 400)
inline int json_number(const std::string & js, const char * key, double & out) {
    const std::string pat = std::string("\"") + key + "\"";
    size_t p = js.find(pat);
    if (p == std::string::npos) return 0;
    p = js.find(':', p + pat.size());
    if (p == std::string::npos) return -1;
    p++;
    while (p < js.size() && (js[p] == ' ' || js[p] == '\t')) p++;
    if (p >= js.size() || !((js[p] >= '0' && js[p] <= '9') || js[p] == '-' || js[p] == '+' || js[p] == '.')) return -1;
    char * end = nullptr;
    out = strtod(js.c_str() + p, &end);
    if (end == js.c_str() + p) return -1;
    return 1;
}
// an integer value (no fraction, within int32): 0 absent, 1 ok, -1 malformed
inline int json_int(const std::string & js, const char * key, int32_t & out) {
    double v = 0.0;
    const int r = json_number(js, key, v);
    if (r <= 0) return r;
    if (!(v >= -2147483648.0 && v <= 2147483647.0) || v != (double) (int64_t) v) return -1;
    out = (int32_t) v;
    return 1;
}
// a float value: 0 absent, 1 ok, -1 malformed (NaN and infinities included)
inline int json_float(const std::string & js, const char * key, float & out) {
    double v = 0.0;
    const int r = json_number(js, key, v);
    if (r <= 0) return r;
    if (!(v >= -3.4e38 && v <= 3.4e38)) return -1;
    out = (float) v;
    return 1;
}

// A voice prompt file (bark.cpp_amd/voice.py writes it), little-endian: "BVP1", int32 n_sem, Tc, Tf, then the int32 arrays semantic [n_sem],
// coarse [Tc][2], fine [Tf][8].
struct VoiceFile { std::vector<int32_t> semantic, coarse, fine; };
inline bool read_voice_file(const std::string & path, VoiceFile & out, std::string & err) {
    FILE * f = fopen(path.c_str(), "rb");
    if (!f) { err = "cannot open " + path; return false; }
    std::vector<char> data;
    char buf[65536];
    size_t k;
    while ((k = fread(buf, 1, sizeof(buf), f)) > 0) data.insert(data.end(), buf, buf + k);
    fclose(f);
    int32_t n[3] = {0, 0, 0};
    if (data.size() < 16 || memcmp(data.data(), "BVP1", 4) != 0) { err = path + ": not a voice prompt file"; return false; }
    memcpy(n, data.data() + 4, 12);
    if (n[0] < 0 || n[1] < 0 || n[2] < 0 || n[0] > (1 << 20) || n[1] > (1 << 20) || n[2] > (1 << 20) ||
        data.size() != 16 + 4 * ((size_t) n[0] + 2 * (size_t) n[1] + 8 * (size_t) n[2])) { err = path + ": counts do not match the file size"; return false; }
    const int32_t * a = reinterpret_cast<const int32_t *>(data.data() + 16);
    out.semantic.assign(a, a + n[0]);
    out.coarse.assign(a + n[0], a + n[0] + 2 * (size_t) n[1]);
    out.fine.assign(a + n[0] + 2 * (size_t) n[1], a + n[0] + 2 * (size_t) n[1] + 8 * (size_t) n[2]);
    return true;
}
// --voice name=file: adds the file to the table; false (err set) on a malformed argument or file
inline bool add_voice(std::map<std::string, VoiceFile> & table, const std::string & arg, std::string & err) {
    const size_t eq = arg.find('=');
    if (eq == std::string::npos || eq == 0 || eq + 1 >= arg.size()) { err = "--voice expects name=file"; return false; }
    VoiceFile v;
    if (!read_voice_file(arg.substr(eq + 1), v, err)) return false;
    table[arg.substr(0, eq)] = std::move(v);
    return true;
}
// the request field "voice": 0 absent (*out = nullptr), 1 *out is the named voice, -1 not a string or an unknown name (a server answers 400)
inline int request_voice(const std::string & js, const std::map<std::string, VoiceFile> & table, const VoiceFile ** out) {
    *out = nullptr;
    if (js.find("\"voice\"") == std::string::npos) return 0;
    std::string name;
    if (!json_string(js, "voice", name)) return -1;
    const auto it = table.find(name);
    if (it == table.end()) return -1;
    *out = &it->second;
    return 1;
}

// the inverse of read_voice_file: the bytes of the file (what bark.cpp_amd/voice.py save() writes), and the file itself
inline std::string voice_file_bytes(const VoiceFile & v) {
    const int32_t n[3] = {(int32_t) v.semantic.size(), (int32_t) (v.coarse.size() / 2), (int32_t) (v.fine.size() / 8)};
    std::string s = "BVP1";
    s.append(reinterpret_cast<const char *>(n), 12);
    s.append(reinterpret_cast<const char *>(v.semantic.data()), (size_t) n[0] * 4);
    s.append(reinterpret_cast<const char *>(v.coarse.data()), (size_t) n[1] * 8);
    s.append(reinterpret_cast<const char *>(v.fine.data()), (size_t) n[2] * 32);
    return s;
}
inline bool write_voice_file(const std::string & path, const VoiceFile & v, std::string & err) {
    if (v.coarse.size() % 2 || v.fine.size() % 8 || v.semantic.size() > (1u << 20) || v.coarse.size() / 2 > (1u << 20) || v.fine.size() / 8 > (1u << 20)) {
        err = "voice prompt: bad array sizes"; return false;
    }
    FILE * f = fopen(path.c_str(), "wb");
    if (!f) { err = "cannot write " + path; return false; }
    const std::string s = voice_file_bytes(v);
    const bool ok = fwrite(s.data(), 1, s.size(), f) == s.size();
    if (fclose(f) != 0 || !ok) { err = "cannot write " + path; return false; }
    return true;
}
// a voice name as a route and a --voice-audio argument take it: 1 .. 64 of [A-Za-z0-9_.-], not starting with a dot
inline bool valid_voice_name(const std::string & name) {
    if (name.empty() || name.size() > 64 || name[0] == '.') return false;
    for (char ch : name) if (!((ch >= 'a' && ch <= 'z') || (ch >= 'A' && ch <= 'Z') || (ch >= '0' && ch <= '9') || ch == '_' || ch == '.' || ch == '-')) return false;
    return true;
}
// the value of `key` in the query string of a request target ("/voices?name=a&x=y" -> "a"); false when the key is absent
inline bool query_param(const std::string & target, const char * key, std::string & out) {
    size_t p = target.find('?');
    while (p != std::string::npos && p + 1 < target.size()) {
        const size_t b = p + 1, e = target.find('&', b), eq = target.find('=', b);
        const size_t end = e == std::string::npos ? target.size() : e;
        if (eq != std::string::npos && eq < end && target.compare(b, eq - b, key) == 0) { out = target.substr(eq + 1, end - eq - 1); return true; }
        p = e;
    }
    return false;
}

// A RIFF / WAVE body -> mono float samples.  Taken: `fmt ` tag 1 (PCM) with 16 bits (x / 32768.0f) or tag 3 (IEEE float) with 32 bits, or tag 0xFFFE
// (extensible) whose sub-format is one of those two; one channel.  Chunks other than `fmt ` and `data` are skipped (an odd size is followed by a pad byte);
// the first `data` chunk is the recording.  Refused with a message: no RIFF / WAVE header, a missing `fmt ` or `data` chunk, a `fmt ` chunk cut short, a
// `data` chunk longer than the body, an empty `data` chunk, more than one channel, any other format.  Nothing is read beyond body.size().
inline bool parse_wav(const std::string & body, std::vector<float> & pcm, int & rate, std::string & err) {
    const size_t size = body.size();
    const unsigned char * d = reinterpret_cast<const unsigned char *>(body.data());
    auto u16 = [&](size_t p) { return (uint32_t) d[p] | ((uint32_t) d[p + 1] << 8); };
    auto u32 = [&](size_t p) { return (uint32_t) d[p] | ((uint32_t) d[p + 1] << 8) | ((uint32_t) d[p + 2] << 16) | ((uint32_t) d[p + 3] << 24); };
    pcm.clear(); rate = 0;
    if (size < 12 || memcmp(d, "RIFF", 4) != 0 || memcmp(d + 8, "WAVE", 4) != 0) { err = "not a RIFF/WAVE file"; return false; }
    bool have_fmt = false, have_data = false;
    uint32_t tag = 0, channels = 0, bits = 0, srate = 0;
    size_t data_at = 0, data_bytes = 0;
    for (size_t pos = 12; pos + 8 <= size && !(have_fmt && have_data);) {
        const size_t at = pos + 8, sz = u32(pos + 4);
        if (memcmp(d + pos, "fmt ", 4) == 0 && !have_fmt) {
            if (sz < 16 || sz > size - at) { err = "the fmt chunk is cut short"; return false; }
            tag = u16(at); channels = u16(at + 2); srate = u32(at + 4); bits = u16(at + 14);
            if (tag == 0xFFFE) {
                static const unsigned char guid_tail[14] = {0x00, 0x00, 0x00, 0x00, 0x10, 0x00, 0x80, 0x00, 0x00, 0xAA, 0x00, 0x38, 0x9B, 0x71};
                if (sz < 40 || u16(at + 16) < 22 || memcmp(d + at + 26, guid_tail, 14) != 0) { err = "unsupported extensible format"; return false; }
                tag = u16(at + 24);
            }
            have_fmt = true;
        } else if (memcmp(d + pos, "data", 4) == 0 && !have_data) {
            if (sz > size - at) { err = "the data chunk is longer than the body"; return false; }
            data_at = at; data_bytes = sz; have_data = true;
        }
        if (sz > size - at) break;                              // an unknown chunk that runs past the body: nothing behind it
        pos = at + sz + (sz & 1);
    }
    if (!have_fmt) { err = "no fmt chunk"; return false; }
    if (!have_data) { err = "no data chunk"; return false; }
    if (channels != 1) { err = "only mono recordings are taken"; return false; }
    if (!((tag == 1 && bits == 16) || (tag == 3 && bits == 32))) { err = "only 16-bit PCM and 32-bit float samples are taken"; return false; }
    if (srate == 0 || srate > 768000) { err = "bad sample rate"; return false; }
    const size_t n = data_bytes / (bits / 8);
    if (n == 0) { err = "the data chunk is empty"; return false; }
    pcm.resize(n);
    if (tag == 1) for (size_t i = 0; i < n; i++) pcm[i] = (float) (int16_t) (uint16_t) u16(data_at + 2 * i) / 32768.0f;
    else memcpy(pcm.data(), d + data_at, n * 4);
    rate = (int) srate;
    return true;
}

// the same over a table whose entries are shared (a server that replaces voices while requests are in flight): *out keeps the voice alive
inline int request_voice(const std::string & js, const std::map<std::string, std::shared_ptr<const VoiceFile>> & table, std::shared_ptr<const VoiceFile> * out) {
    out->reset();
    if (js.find("\"voice\"") == std::string::npos) return 0;
    std::string name;
    if (!json_string(js, "voice", name)) return -1;
    const auto it = table.find(name);
    if (it == table.end()) return -1;
    *out = it->second;
    return 1;
}

inline std::string wav_f32(const float * pcm, int n, int rate) {
    auto u32 = [](std::string & s, uint32_t v) { s.append(reinterpret_cast<const char *>(&v), 4); };
    auto u16 = [](std::string & s, uint16_t v) { s.append(reinterpret_cast<const char *>(&v), 2); };
    std::string s;
    const uint32_t bytes = (uint32_t) n * 4;
    s += "RIFF"; u32(s, 36 + bytes); s += "WAVE";
    s += "fmt "; u32(s, 16); u16(s, 3 /* IEEE float */); u16(s, 1); u32(s, (uint32_t) rate); u32(s, (uint32_t) rate * 4); u16(s, 4); u16(s, 32);
    s += "data"; u32(s, bytes);
    s.append(reinterpret_cast<const char *>(pcm), bytes);
    return s;
}

// the request field / option value "f32" | "s16" | "mulaw" | "flac" -> 0 | 1 | 2 | 3 (enum bark_hip_sample_format and BARK_HIP_SAMPLE_FLAC), -1: anything else
inline int sample_format_of(const std::string & name) { return name == "f32" ? 0 : name == "s16" ? 1 : name == "mulaw" ? 2 : name == "flac" ? 3 : -1; }
// A /bark request's "sample_rate" / "format" over the server's defaults in (rate, format): false for a field of the wrong type or a format name that is none
// of the four (whether the engine serves the rate is the caller's check)
inline bool request_format(const std::string & js, int32_t & rate, int32_t & format) {
    if (json_int(js, "sample_rate", rate) < 0) return false;
    if (js.find("\"format\"") != std::string::npos) {
        std::string name;
        format = json_string(js, "format", name) ? sample_format_of(name) : -1;
    }
    return format >= 0 && format <= 3;
}
// what an answer in `format` is served as: FLAC (3, rule C18f) is a complete stream and goes out as it is, everything else inside a WAV
inline const char * answer_type(int format) { return format == 3 ? "audio/flac" : "audio/wav"; }

// A mono WAV around n samples in one of the three sample formats: 0 IEEE float (tag 3, 32 bit; the bytes of wav_f32), 1 PCM (tag 1, 16 bit), 2 G.711 mu-law
// (tag 7, 8 bit: a non-PCM format, so the fmt chunk carries cbSize = 0 and a `fact` chunk states the sample count; an odd data chunk is followed by a pad byte)
inline std::string wav_samples(const void * data, int n, int rate, int format) {
    auto u32 = [](std::string & s, uint32_t v) { s.append(reinterpret_cast<const char *>(&v), 4); };
    auto u16 = [](std::string & s, uint16_t v) { s.append(reinterpret_cast<const char *>(&v), 2); };
    if (format == 0) return wav_f32(static_cast<const float *>(data), n, rate);
    const uint32_t width = format == 1 ? 2 : 1, bytes = (uint32_t) n * width, pad = bytes & 1;
    std::string s;
    s += "RIFF"; u32(s, (format == 1 ? 36 : 50) + bytes + pad); s += "WAVE";
    s += "fmt "; u32(s, format == 1 ? 16 : 18); u16(s, format == 1 ? 1 /* PCM */ : 7 /* mu-law */); u16(s, 1); u32(s, (uint32_t) rate); u32(s, (uint32_t) rate * width);
    u16(s, (uint16_t) width); u16(s, (uint16_t) (8 * width));
    if (format != 1) { u16(s, 0); s += "fact"; u32(s, 4); u32(s, (uint32_t) n); }
    s += "data"; u32(s, bytes);
    s.append(static_cast<const char *>(data), bytes);
    if (pad) s.push_back('\0');
    return s;
}

}  // namespace barkhttp
