// batcher.hip - a native request collector in front of bark_hip_generate_batch.
//
// The reference's HTTP example serialises its requests on one mutex around bark_generate_audio (examples/server/server.cpp:76-94,
// 128-163): one utterance in flight, every decode step streams the weights for a single sequence.  This component is what a server puts
// in that place on this engine: any number of host threads submit texts; ONE worker thread owns the context, collects what is pending
// (up to max_batch requests, waiting at most max_wait_ms for a batch to fill once the first request is there) and runs them as one
// lock-step batch.  Per-request results are those of a fresh context seeded with the request's seed (engine_generate_batch's contract),
// whatever batch a request happened to travel in.  Plain C++ threads; the device is touched through the engine's entry points only, on the worker that owns the context.
// A request may ask for its answer in another rate / sample format (bark_hip_batcher_submit_as, rule C14r): the worker converts behind the job, one
// engine_resample_many per distinct format among the job's requests; requests in {24000, f32} take the path they always took.
// A long text (bark_hip_batcher_submit_long, rules C15s / C15j) is one ticket over several ordinary requests: the worker that finishes the last of them
// joins their audio with engine_join_many on its own context.
// A request may carry a speaking rate (bark_hip_batcher_submit_at, rule C16t): behind the job the worker runs one engine_tempo_many over all its requests with
// a speed other than 1000 (64 segments a call), and the conversion above then reads the time-scaled samples; a long text's parts are time-scaled in front of
// its join.  Speed 1000 takes the path it always took.
// A request may ask for a loudness (bark_hip_batcher_submit_with, rule C17l): the same call behind the job becomes engine_level_many over all its requests with
// levelling on or a speed other than 1000 - one measure launch and one level launch in front of the single tempo launch; a long text's parts are levelled, each
// on its own, in front of tempo and join.  Levelling off takes the path it always took.
// A request may ask for BARK_HIP_SAMPLE_FLAC (rule C18f): the conversion above then runs the encoder's two launches behind its format launch, once for
// all requests of the job at that rate, and only the streams return to the host; a long text's ticket is one stream over its joined audio.
// Job streams (bark_hip_batcher_create_ex, n_streams 1 .. 4): further workers on clones of the context (own streams, caches and graphs, the
// same weights) serve the same queue - a lock step is a chain of ~100 small dependent kernels, so two jobs share the chip (two streams of
// 64-slot jobs out of phase: 37.8 prompts/s against 33.2 from one, profiles/r04_staggered_jobs.txt).  Workers that start together stay in
// phase, so the first job of worker i > 0 is capped at max_batch / 2: the streams then run about half a job apart.
#include "engine_internal.h"

#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <thread>
#include <unordered_map>

using namespace barkhip;

struct bark_hip_batcher {
    struct Req;
    // A long text (bark_hip_batcher_submit_long, rules C15s / C15j): its parts are ordinary requests in the queue - they share jobs with other traffic and
    // may be served by different workers - and `whole` is what the ticket waits for.  `left` counts the parts still out and is only touched under `mu`:
    // the worker that brings it to zero joins the parts' audio on its own context.
    struct Long { std::vector<std::shared_ptr<Req>> parts; std::shared_ptr<Req> whole; int left = 0; bool failed = false; bark_hip_join_params join{6000, 0, 0.0f, 0}; };
    struct Req {
        std::shared_ptr<Long> of;                                   // a part of a long text: not in `tickets`, its audio goes to the join
        std::string text; bark_hip_request_params rp{}; bark_hip_sampling_filter flt{0, 1.0f}; VoicePtr voice; std::vector<float> pcm; bool done = false, ok = false;
        bark_hip_audio_format fmt{24000, BARK_HIP_SAMPLE_F32};      // what the answer comes in (bark_hip_batcher_submit_as); the default keeps pcm, any other fills bytes
        std::vector<uint8_t> bytes;
        int n_parts = 1;                                            // the parts a long text's ticket stands for (bark_hip_batcher_ticket_chunks)
        int speed = 1000;                                           // speaking rate in per mille (bark_hip_batcher_submit_at); a long text's ticket carries it, its parts do not
        bark_hip_loudness_params loud{0, 0.0f, 0.0f};               // levelling (bark_hip_batcher_submit_with; target 0: none), carried like the speed
        bool rendered() const { return speed != 1000 || loud.target_centilufs != 0; }
        bool plain() const { return fmt.sample_rate == 24000 && fmt.sample_format == BARK_HIP_SAMPLE_F32; }
    };
    bark_context * ctx = nullptr;                          // worker 0's context (the caller's); request defaults are read from it
    std::vector<bark_context *> ctxs;                      // one per worker; ctxs[1 ..] are clones owned by the batcher ...
    bool owns_workers = true;                              // ... unless the caller brought every context itself (bark_hip_batcher_create_multi: one per GPU)
    // the context's top-k / nucleus filter, copied when the collector is made (the workers own the contexts from then on): what a request without a
    // filter of its own gets, read under `mu` at submit time - nothing is ever written into a running worker's context
    bark_hip_sampling_filter default_filter{0, 1.0f};
    VoicePtr default_voice;                                // the context's voice prompt, copied the same way (requests without a voice of their own)
    int max_batch = 32;
    std::chrono::microseconds max_wait{2000};
    std::mutex mu;
    std::condition_variable cv_work, cv_done;
    std::deque<std::pair<int64_t, std::shared_ptr<Req>>> queue;
    std::unordered_map<int64_t, std::shared_ptr<Req>> tickets;
    int64_t next_ticket = 1;
    bool stop = false;
    int n_batches = 0, n_requests = 0, largest = 0, n_admitted = 0;      // n_admitted: requests that joined a running job
    std::vector<std::thread> workers;

    void run(int wi) {
        bark_context * ctx = ctxs[(size_t) wi];
        bool first = wi > 0 && owns_workers;              // job streams on ONE GPU are kept out of phase (file header); workers on GPUs of their own need not be
        std::unique_lock<std::mutex> lk(mu);
        while (true) {
            cv_work.wait(lk, [&] { return stop || !queue.empty(); });
            if (stop && queue.empty()) return;
            // the first request is there: give the batch max_wait to fill (a full batch leaves at once)
            const auto deadline = std::chrono::steady_clock::now() + max_wait;
            cv_work.wait_until(lk, deadline, [&] { return stop || (int) queue.size() >= max_batch; });
            const int job_cap = first ? std::max(1, max_batch / 2) : max_batch;       // de-phases the job streams (see the file header)
            first = false;
            std::vector<std::shared_ptr<Req>> batch;
            while (!queue.empty() && (int) batch.size() < job_cap) { batch.push_back(queue.front().second); queue.pop_front(); }
            if (batch.empty()) continue;                         // another worker took what was there
            lk.unlock();
            std::vector<const char *> texts; std::vector<bark_hip_request_params> rps; std::vector<bark_hip_sampling_filter> flts; std::vector<VoicePtr> voices;
            for (auto & r : batch) { texts.push_back(r->text.c_str()); rps.push_back(r->rp); flts.push_back(r->flt); voices.push_back(r->voice); }
            // every request carries its voice (or none): the worker's own context must not add one of its own
            const VoicePtr ctx_voice = ctx->voice;
            ctx->voice.reset();
            // continuous admission: requests that arrive while the job's semantic stage has free slots join it (engine_generate_batch asks here)
            BatchAdmit admit;
            admit.max_job = job_cap;
            admit.next = [&](std::string & text, bark_hip_request_params & rp, bark_hip_sampling_filter & flt, VoicePtr & voice) {
                std::lock_guard<std::mutex> g(mu);
                if (queue.empty() || (int) batch.size() >= job_cap) return false;
                batch.push_back(queue.front().second); queue.pop_front();
                text = batch.back()->text; rp = batch.back()->rp; flt = batch.back()->flt; voice = batch.back()->voice;
                n_admitted++;
                return true;
            };
            bool failed = false;
            try { engine_generate_batch(ctx, texts.data(), (int) texts.size(), nullptr, rps.data(), &admit, flts.data(), voices.data()); }
            catch (const std::exception & e) { fprintf(stderr, "bark_hip_batcher: batch failed: %s\n", e.what()); failed = true; }
            ctx->voice = ctx_voice;
            // answers at another speaking rate or level: ONE tempo launch over all of them (64 segments a call), behind one measure and one level launch if any
            // of them levels; 24 kHz f32 out; what follows reads `scaled` for these
            std::vector<std::vector<float>> scaled(batch.size());
            std::vector<char> scaled_ok(batch.size(), 0);
            auto has_audio = [&](size_t i) { return i < ctx->batch_results.size() && ctx->batch_results[i].ok && !ctx->batch_results[i].audio.empty(); };
            std::vector<size_t> fast;
            for (size_t i = 0; i < batch.size() && !failed; i++) if (batch[i]->rendered() && has_audio(i)) fast.push_back(i);
            for (size_t g0 = 0; g0 < fast.size(); g0 += kResampleMaxSegments) {
                const size_t g1 = std::min(fast.size(), g0 + (size_t) kResampleMaxSegments);
                std::vector<const float *> ptr; std::vector<int> len; std::vector<int32_t> sp, n_out; std::vector<bark_hip_loudness_params> loud;
                bool levels = false;
                for (size_t g = g0; g < g1; g++) {
                    ptr.push_back(ctx->batch_results[fast[g]].audio.data()); len.push_back((int) ctx->batch_results[fast[g]].audio.size()); sp.push_back(batch[fast[g]]->speed);
                    loud.push_back(batch[fast[g]]->loud); levels = levels || loud.back().target_centilufs != 0;
                }
                try {
                    const std::vector<uint8_t> r = levels ? engine_level_many(ctx, ptr.data(), len.data(), (int) ptr.size(), loud.data(), sp.data(), 24000, BARK_HIP_SAMPLE_F32, n_out)
                                                          : engine_tempo_many(ctx, ptr.data(), len.data(), (int) ptr.size(), sp.data(), 24000, BARK_HIP_SAMPLE_F32, n_out);
                    size_t off = 0;
                    for (size_t g = g0; g < g1; g++) {
                        const size_t nb = (size_t) n_out[g - g0] * sizeof(float);
                        scaled[fast[g]].resize((size_t) n_out[g - g0]); memcpy(scaled[fast[g]].data(), r.data() + off, nb); scaled_ok[fast[g]] = 1; off += nb;
                    }
                } catch (const std::exception & e) { fprintf(stderr, "bark_hip_batcher: time scaling failed: %s\n", e.what()); }
            }
            // the 24 kHz f32 samples request i answers with: its result, or the time-scaled form of it (empty: none)
            auto source = [&](size_t i) -> const std::vector<float> & {
                static const std::vector<float> none;
                if (!has_audio(i)) return none;
                return !batch[i]->rendered() ? ctx->batch_results[i].audio : (scaled_ok[i] ? scaled[i] : none);
            };
            // answers in another rate / format: converted here, on the thread that owns the context, one resample_many per distinct format (64 segments a call)
            std::vector<std::vector<uint8_t>> conv(batch.size());
            std::vector<char> conv_ok(batch.size(), 0);
            for (size_t i = 0; i < batch.size() && !failed; i++) {
                if (batch[i]->plain() || conv_ok[i] || source(i).empty()) continue;
                const bark_hip_audio_format f = batch[i]->fmt;
                std::vector<size_t> who;
                for (size_t k = i; k < batch.size(); k++)
                    if (!batch[k]->plain() && batch[k]->fmt.sample_rate == f.sample_rate && batch[k]->fmt.sample_format == f.sample_format && !source(k).empty() && !conv_ok[k])
                        who.push_back(k);
                for (size_t g0 = 0; g0 < who.size(); g0 += kResampleMaxSegments) {
                    const size_t g1 = std::min(who.size(), g0 + (size_t) kResampleMaxSegments);
                    std::vector<const float *> ptr; std::vector<int> len; std::vector<int32_t> n_out;
                    for (size_t g = g0; g < g1; g++) { ptr.push_back(source(who[g]).data()); len.push_back((int) source(who[g]).size()); }
                    try {
                        const std::vector<uint8_t> r = engine_resample_many(ctx, ptr.data(), len.data(), (int) ptr.size(), 24000, f.sample_rate, f.sample_format, n_out);
                        size_t off = 0;
                        for (size_t g = g0; g < g1; g++) {
                            const size_t nb = f.sample_format == BARK_HIP_SAMPLE_FLAC ? (size_t) ctx->flac_lengths[g - g0]      // a stream per request (rule C18f)
                                                                                      : (size_t) n_out[g - g0] * (size_t) sample_format_bytes(f.sample_format);
                            conv[who[g]].assign(r.begin() + (long) off, r.begin() + (long) (off + nb)); conv_ok[who[g]] = 1; off += nb;
                        }
                    } catch (const std::exception & e) { fprintf(stderr, "bark_hip_batcher: conversion failed: %s\n", e.what()); }
                }
            }
            lk.lock();
            std::vector<std::shared_ptr<Long>> to_join;             // long texts whose LAST part this job finished ("last" is decided here, under mu)
            for (size_t i = 0; i < batch.size(); i++) {
                Req & r = *batch[i];
                if (!failed && i < ctx->batch_results.size() && ctx->batch_results[i].ok) {
                    if (r.plain()) { r.pcm = source(i); r.ok = !r.rendered() || scaled_ok[i]; }
                    else if (conv_ok[i]) { r.bytes = std::move(conv[i]); r.ok = true; }
                }
                r.done = true;
                if (r.of) {
                    if (!r.ok || r.pcm.empty()) r.of->failed = true;
                    if (--r.of->left == 0) to_join.push_back(r.of);
                }
            }
            n_batches++; n_requests += (int) batch.size(); largest = std::max(largest, (int) batch.size());
            cv_done.notify_all();
            // the join of a finished long text, on this worker's context: nobody else touches its parts any more (left == 0), so the lock is not held meanwhile
            for (auto & lg : to_join) {
                lk.unlock();
                Req & w = *lg->whole;
                bool ok = !lg->failed;
                if (ok) {
                    std::vector<const float *> ptr; std::vector<int> len; std::vector<int32_t> layout;
                    for (auto & p : lg->parts) { ptr.push_back(p->pcm.data()); len.push_back((int) p->pcm.size()); }
                    try {
                        std::vector<uint8_t> fast_parts;            // the parts at the ticket's speaking rate (rule C16t: the join runs over the time-scaled chunks)
                        if (w.rendered()) {                        // .. and level (rule C17l: each part on its own, in front of the tempo)
                            const std::vector<int32_t> sp(ptr.size(), w.speed);
                            const std::vector<bark_hip_loudness_params> loud(ptr.size(), w.loud);
                            std::vector<int32_t> n24;
                            fast_parts = w.loud.target_centilufs != 0
                                ? engine_level_many(ctx, ptr.data(), len.data(), (int) ptr.size(), loud.data(), sp.data(), 24000, BARK_HIP_SAMPLE_F32, n24)
                                : engine_tempo_many(ctx, ptr.data(), len.data(), (int) ptr.size(), sp.data(), 24000, BARK_HIP_SAMPLE_F32, n24);
                            size_t off = 0;
                            for (size_t i = 0; i < ptr.size(); i++) { ptr[i] = reinterpret_cast<const float *>(fast_parts.data()) + off; len[i] = n24[i]; off += (size_t) n24[i]; }
                        }
                        std::vector<uint8_t> joined = engine_join_many(ctx, ptr.data(), len.data(), (int) ptr.size(), lg->join, w.fmt.sample_rate, w.fmt.sample_format, layout);
                        if (w.plain()) { w.pcm.resize(joined.size() / sizeof(float)); if (!joined.empty()) memcpy(w.pcm.data(), joined.data(), joined.size()); }
                        else w.bytes = std::move(joined);
                    } catch (const std::exception & e) { fprintf(stderr, "bark_hip_batcher: join failed: %s\n", e.what()); ok = false; }
                }
                lk.lock();
                lg->parts.clear();
                w.ok = ok; w.done = true;
                cv_done.notify_all();
            }
        }
    }
};

extern "C" {

BARK_API struct bark_hip_batcher * bark_hip_batcher_create_ex(struct bark_context * bctx, int max_batch, int max_wait_ms, int n_streams) {
    if (!bctx || max_batch < 1 || max_batch > 256 || max_wait_ms < 0 || n_streams < 1 || n_streams > 4) return nullptr;
    std::unique_ptr<bark_hip_batcher> b(new bark_hip_batcher());
    try {
        b->ctx = bctx; b->max_batch = max_batch; b->max_wait = std::chrono::microseconds((int64_t) max_wait_ms * 1000);
        b->default_filter = bctx->filter;
        b->default_voice = bctx->voice;
        b->ctxs.push_back(bctx);
        for (int i = 1; i < n_streams; i++) {
            b->ctxs.push_back(engine_clone(bctx, (uint32_t) i));
            // the progress callback belongs to the thread that calls into the context (bark.h contract): the further job streams run on
            // threads of their own, so they report nothing instead of calling the user's function concurrently with the same user_data
            b->ctxs.back()->params.progress_callback = nullptr; b->ctxs.back()->params.progress_callback_user_data = nullptr;
        }
        for (bark_context * c : b->ctxs) engine_reserve_batch(c, std::min(max_batch, 64));   // the slot count is fixed by the first use; a larger job queues for the slots
        bark_hip_batcher * raw = b.get();
        for (int i = 0; i < n_streams; i++) b->workers.emplace_back([raw, i] { raw->run(i); });
        return b.release();
    } catch (const std::exception & e) {
        fprintf(stderr, "bark_hip_batcher_create: %s\n", e.what());
        // workers that did start must be joined before the object goes away (a joinable std::thread's destructor terminates the process)
        { std::lock_guard<std::mutex> lk(b->mu); b->stop = true; b->cv_work.notify_all(); }
        for (auto & w : b->workers) if (w.joinable()) w.join();
        for (size_t i = 1; i < b->ctxs.size(); i++) delete b->ctxs[i];
        return nullptr;
    }
}
// Several GPUs behind ONE queue (north_star: many prompts sharded across the GPUs of a node as an embarrassingly-parallel split, no collective inside an
// utterance - here natively, without torch.distributed): worker i is the caller's context i, typically loaded on device i with
// bark_hip_load_model_on_device; every engine entry point selects its context's device first, so a worker thread needs no device state of its own.
// The collector does not own these contexts (bark_free them after bark_hip_batcher_free).  Request defaults are read from ctxs[0].
BARK_API struct bark_hip_batcher * bark_hip_batcher_create_multi(struct bark_context * const * ctxs, int n_ctx, int max_batch, int max_wait_ms) {
    if (!ctxs || n_ctx < 1 || n_ctx > 64 || max_batch < 1 || max_batch > 256 || max_wait_ms < 0) return nullptr;
    for (int i = 0; i < n_ctx; i++) {
        if (!ctxs[i]) return nullptr;
        for (int j = 0; j < i; j++) if (ctxs[j] == ctxs[i]) return nullptr;            // one worker per context
    }
    std::unique_ptr<bark_hip_batcher> b(new bark_hip_batcher());
    try {
        b->ctx = ctxs[0]; b->max_batch = max_batch; b->max_wait = std::chrono::microseconds((int64_t) max_wait_ms * 1000);
        b->default_filter = ctxs[0]->filter;
        b->default_voice = ctxs[0]->voice;
        b->owns_workers = false;
        for (int i = 0; i < n_ctx; i++) b->ctxs.push_back(ctxs[i]);
        for (bark_context * c : b->ctxs) engine_reserve_batch(c, std::min(max_batch, 64));
        bark_hip_batcher * raw = b.get();
        for (int i = 0; i < n_ctx; i++) b->workers.emplace_back([raw, i] { raw->run(i); });
        return b.release();
    } catch (const std::exception & e) {
        fprintf(stderr, "bark_hip_batcher_create_multi: %s\n", e.what());
        { std::lock_guard<std::mutex> lk(b->mu); b->stop = true; b->cv_work.notify_all(); }
        for (auto & w : b->workers) if (w.joinable()) w.join();
        return nullptr;
    }
}
BARK_API struct bark_hip_batcher * bark_hip_batcher_create(struct bark_context * bctx, int max_batch, int max_wait_ms) {
    return bark_hip_batcher_create_ex(bctx, max_batch, max_wait_ms, 1);
}

static int64_t batcher_enqueue(struct bark_hip_batcher * b, const char * text, const bark_hip_request_params & rp, const bark_hip_sampling_filter * flt = nullptr,
                               const VoicePtr * voice = nullptr, const bark_hip_audio_format * fmt = nullptr, int speed = 1000,
                               const bark_hip_loudness_params & loud = bark_hip_loudness_params{0, 0.0f, 0.0f}) {
    auto r = std::make_shared<bark_hip_batcher::Req>();
    r->text = text; r->rp = rp; r->speed = speed; r->loud = loud;
    if (fmt) r->fmt = *fmt;
    std::lock_guard<std::mutex> lk(b->mu);
    if (b->stop) return -1;
    r->flt = flt ? *flt : b->default_filter;
    r->voice = voice ? *voice : b->default_voice;
    const int64_t t = b->next_ticket++;
    b->tickets[t] = r;
    b->queue.emplace_back(t, r);
    b->cv_work.notify_all();
    return t;
}
static bark_hip_request_params context_request_params(const bark_context * c, uint32_t seed) {
    bark_hip_request_params rp{};
    rp.temp = c->params.temp; rp.fine_temp = c->params.fine_temp; rp.min_eos_p = c->params.min_eos_p; rp.n_steps_text_encoder = c->params.n_steps_text_encoder; rp.seed = seed;
    return rp;
}
BARK_API int64_t bark_hip_batcher_submit(struct bark_hip_batcher * b, const char * text, uint32_t seed) {
    if (!b || !text) return -1;
    return batcher_enqueue(b, text, context_request_params(b->ctx, seed));
}
BARK_API int64_t bark_hip_batcher_submit_ex(struct bark_hip_batcher * b, const char * text, const struct bark_hip_request_params * params) {
    if (!b || !text) return -1;
    return batcher_enqueue(b, text, params ? *params : context_request_params(b->ctx, 0));
}
BARK_API int64_t bark_hip_batcher_submit_filtered(struct bark_hip_batcher * b, const char * text, const struct bark_hip_request_params * params,
                                                  const struct bark_hip_sampling_filter * filter) {
    if (!b || !text || (filter && !filter_valid(*filter))) return -1;
    return batcher_enqueue(b, text, params ? *params : context_request_params(b->ctx, 0), filter);
}
BARK_API int64_t bark_hip_batcher_submit_voiced(struct bark_hip_batcher * b, const char * text, const struct bark_hip_request_params * params,
                                                const struct bark_hip_sampling_filter * filter, const struct bark_hip_voice_prompt * voice) {
    if (!b || !text || (filter && !filter_valid(*filter))) return -1;
    VoicePtr v;
    if (voice) {
        // checked against the collector's context as it was made (parameters and models are fixed while the collector lives); copies the arrays
        try { v = engine_make_voice(b->ctx, voice); }
        catch (const std::exception & e) { fprintf(stderr, "bark_hip_batcher_submit_voiced: %s\n", e.what()); return -1; }
    }
    return batcher_enqueue(b, text, params ? *params : context_request_params(b->ctx, 0), filter, voice ? &v : nullptr);
}

BARK_API int64_t bark_hip_batcher_submit_as(struct bark_hip_batcher * b, const char * text, const struct bark_hip_request_params * params,
                                            const struct bark_hip_sampling_filter * filter, const struct bark_hip_voice_prompt * voice,
                                            const struct bark_hip_audio_format * fmt) {
    return bark_hip_batcher_submit_at(b, text, params, filter, voice, fmt, 1000);
}
BARK_API int64_t bark_hip_batcher_submit_at(struct bark_hip_batcher * b, const char * text, const struct bark_hip_request_params * params,
                                            const struct bark_hip_sampling_filter * filter, const struct bark_hip_voice_prompt * voice,
                                            const struct bark_hip_audio_format * fmt, int speed_permille) {
    const bark_hip_audio_render how{fmt ? *fmt : bark_hip_audio_format{24000, BARK_HIP_SAMPLE_F32}, speed_permille, {0, 0.0f, 0.0f}};
    return bark_hip_batcher_submit_with(b, text, params, filter, voice, &how);
}
BARK_API int64_t bark_hip_batcher_submit_with(struct bark_hip_batcher * b, const char * text, const struct bark_hip_request_params * params,
                                              const struct bark_hip_sampling_filter * filter, const struct bark_hip_voice_prompt * voice,
                                              const struct bark_hip_audio_render * how) {
    if (!b || !text || !how || (filter && !filter_valid(*filter)) || how->speed_permille < kTempoMinSpeed || how->speed_permille > kTempoMaxSpeed) return -1;
    if (!loudness_params_valid(how->loudness) || !render_format_bytes(how->fmt.sample_format) || !resample_pair_supported(24000, how->fmt.sample_rate)) return -1;
    VoicePtr v;
    if (voice) {
        try { v = engine_make_voice(b->ctx, voice); }
        catch (const std::exception & e) { fprintf(stderr, "bark_hip_batcher_submit_as: %s\n", e.what()); return -1; }
    }
    return batcher_enqueue(b, text, params ? *params : context_request_params(b->ctx, 0), filter, voice ? &v : nullptr, &how->fmt, how->speed_permille, how->loudness);
}

// A long text as ONE ticket (rules C15s / C15j): split here, on the caller's thread (the vocabulary is immutable); the parts enter the queue as ordinary
// requests - part i with seed params->seed + i - so they share jobs with other traffic and continuous admission applies; the worker that finishes the
// last part joins.  Only chain == 0: a chained chunk needs the one before it, which is a sequence of jobs, not a job.
BARK_API int64_t bark_hip_batcher_submit_long(struct bark_hip_batcher * b, const char * text, const struct bark_hip_long_params * long_params,
                                              const struct bark_hip_request_params * params, const struct bark_hip_sampling_filter * filter,
                                              const struct bark_hip_voice_prompt * voice, const struct bark_hip_audio_format * fmt) {
    return bark_hip_batcher_submit_long_at(b, text, long_params, params, filter, voice, fmt, 1000);
}
BARK_API int64_t bark_hip_batcher_submit_long_at(struct bark_hip_batcher * b, const char * text, const struct bark_hip_long_params * long_params,
                                                 const struct bark_hip_request_params * params, const struct bark_hip_sampling_filter * filter,
                                                 const struct bark_hip_voice_prompt * voice, const struct bark_hip_audio_format * fmt, int speed_permille) {
    const bark_hip_audio_render how{fmt ? *fmt : bark_hip_audio_format{24000, BARK_HIP_SAMPLE_F32}, speed_permille, {0, 0.0f, 0.0f}};
    return bark_hip_batcher_submit_long_with(b, text, long_params, params, filter, voice, &how);
}
BARK_API int64_t bark_hip_batcher_submit_long_with(struct bark_hip_batcher * b, const char * text, const struct bark_hip_long_params * long_params,
                                                   const struct bark_hip_request_params * params, const struct bark_hip_sampling_filter * filter,
                                                   const struct bark_hip_voice_prompt * voice, const struct bark_hip_audio_render * how) {
    if (!b || !text || !how || (filter && !filter_valid(*filter)) || how->speed_permille < kTempoMinSpeed || how->speed_permille > kTempoMaxSpeed) return -1;
    if (!loudness_params_valid(how->loudness) || !render_format_bytes(how->fmt.sample_format) || !resample_pair_supported(24000, how->fmt.sample_rate)) return -1;
    const bark_hip_long_params lp = long_params ? *long_params : bark_hip_long_params{0, 0, join_default_params()};
    if (lp.chain != 0 || !join_params_valid(lp.join)) return -1;
    VoicePtr v;
    std::vector<TextSpan> spans;
    const std::string full(text);
    try {
        if (voice) v = engine_make_voice(b->ctx, voice);
        spans = split_text(b->ctx->vocab, full, lp.max_tokens);
    } catch (const std::exception & e) { fprintf(stderr, "bark_hip_batcher_submit_long: %s\n", e.what()); return -1; }
    if (spans.empty()) spans.push_back({0, (int32_t) full.size()});      // a text without a word runs as one part
    const bark_hip_request_params rp = params ? *params : context_request_params(b->ctx, 0);
    auto lg = std::make_shared<bark_hip_batcher::Long>();
    lg->join = lp.join; lg->left = (int) spans.size();
    lg->whole = std::make_shared<bark_hip_batcher::Req>();
    lg->whole->n_parts = (int) spans.size();
    lg->whole->fmt = how->fmt;
    lg->whole->speed = how->speed_permille;
    lg->whole->loud = how->loudness;
    for (size_t i = 0; i < spans.size(); i++) {
        auto r = std::make_shared<bark_hip_batcher::Req>();
        r->of = lg; r->text = full.substr((size_t) spans[i].begin, (size_t) (spans[i].end - spans[i].begin)); r->rp = rp; r->rp.seed = rp.seed + (uint32_t) i;
        lg->parts.push_back(r);
    }
    std::lock_guard<std::mutex> lk(b->mu);
    if (b->stop) { lg->parts.clear(); return -1; }
    const int64_t t = b->next_ticket++;
    b->tickets[t] = lg->whole;
    for (auto & r : lg->parts) {
        r->flt = filter ? *filter : b->default_filter;
        r->voice = voice ? v : b->default_voice;
        b->queue.emplace_back(t, r);
    }
    b->cv_work.notify_all();
    return t;
}

BARK_API int bark_hip_batcher_ticket_chunks(struct bark_hip_batcher * b, int64_t ticket) {
    if (!b) return -1;
    std::lock_guard<std::mutex> lk(b->mu);
    auto it = b->tickets.find(ticket);
    return it == b->tickets.end() ? -1 : it->second->n_parts;
}

BARK_API int bark_hip_batcher_wait_bytes(struct bark_hip_batcher * b, int64_t ticket, void * out, int capacity_bytes) {
    if (!b) return -1;
    std::unique_lock<std::mutex> lk(b->mu);
    auto it = b->tickets.find(ticket);
    if (it == b->tickets.end()) return -1;
    std::shared_ptr<bark_hip_batcher::Req> r = it->second;
    b->cv_done.wait(lk, [&] { return r->done; });
    if (!r->ok) { b->tickets.erase(ticket); return -1; }
    const void * src = r->plain() ? (const void *) r->pcm.data() : (const void *) r->bytes.data();
    const size_t bytes = r->plain() ? r->pcm.size() * sizeof(float) : r->bytes.size();
    if (!out || (size_t) std::max(capacity_bytes, 0) < bytes) return -2 - (int) bytes;      // too small: -(2 + bytes); the ticket stays valid
    memcpy(out, src, bytes);
    b->tickets.erase(ticket);
    return (int) bytes;
}

BARK_API int bark_hip_batcher_wait(struct bark_hip_batcher * b, int64_t ticket, float * pcm, int capacity) {
    if (!b) return -1;
    std::unique_lock<std::mutex> lk(b->mu);
    auto it = b->tickets.find(ticket);
    if (it == b->tickets.end()) return -1;
    std::shared_ptr<bark_hip_batcher::Req> r = it->second;
    if (!r->plain()) return -1;                                 // its answer is not 24 kHz f32: bark_hip_batcher_wait_bytes; the ticket stays valid
    b->cv_done.wait(lk, [&] { return r->done; });
    if (!r->ok) { b->tickets.erase(ticket); return -1; }
    if (!pcm || capacity < (int) r->pcm.size()) return -2 - (int) r->pcm.size();       // too small: -(2 + samples); the ticket stays valid
    memcpy(pcm, r->pcm.data(), r->pcm.size() * sizeof(float));
    const int n = (int) r->pcm.size();
    b->tickets.erase(ticket);
    return n;
}

BARK_API void bark_hip_batcher_stats(struct bark_hip_batcher * b, int * n_batches, int * n_requests, int * largest_batch) {
    if (!b) return;
    std::lock_guard<std::mutex> lk(b->mu);
    if (n_batches) *n_batches = b->n_batches;
    if (n_requests) *n_requests = b->n_requests;
    if (largest_batch) *largest_batch = b->largest;
}

BARK_API int bark_hip_batcher_admitted(struct bark_hip_batcher * b) {
    if (!b) return -1;
    std::lock_guard<std::mutex> lk(b->mu);
    return b->n_admitted;
}

BARK_API void bark_hip_batcher_free(struct bark_hip_batcher * b) {
    if (!b) return;
    { std::lock_guard<std::mutex> lk(b->mu); b->stop = true; b->cv_work.notify_all(); }
    for (auto & w : b->workers) if (w.joinable()) w.join();    // pending requests are still served
    { std::lock_guard<std::mutex> lk(b->mu); b->tickets.clear(); }   // tickets nobody waited for
    if (b->owns_workers) for (size_t i = 1; i < b->ctxs.size(); i++) delete b->ctxs[i];
    delete b;
}

}  // extern "C"
