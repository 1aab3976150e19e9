// native_stage.hpp -- part of mirge_native.hip (one translation unit): what the exporters that write a file straight from the resident
// run share (`--sam-out`, `--sorted-bam`, `--coverage`, `--coverage-bigwig`).  Their output never exists whole: it is produced chunk by
// chunk on the device, copied into one of the two halves of the context's page-locked staging (mirge_ctx::stage_pinned, kept between
// calls) and put into the file (OutFile, native_host.hpp) while the next chunk is being produced.  StagePipe is that loop and owns
// its two events; env_bytes reads the exporters' MIRGE_* sizes.
#pragma once

static size_t env_bytes(const char* name, size_t dflt) {
    const char* v = std::getenv(name);
    if (!v || !*v) return dflt;
    const long long x = std::atoll(v);
    return x > 0 ? (size_t)x : dflt;
}

struct StagePipe {
    mirge_ctx* c;
    std::string who, lost;  // lost: what is said when the wait for a chunk fails
    size_t per_half = 0;
    hipEvent_t ev[2];
    StagePipe(mirge_ctx* c_, std::string w, std::string l = "the copy of a chunk failed") : c(c_), who(std::move(w)), lost(std::move(l)) {
        ev[0] = c->get_evt(); ev[1] = c->get_evt();
    }
    StagePipe(const StagePipe&) = delete;
    StagePipe& operator=(const StagePipe&) = delete;
    // the stream is idle before the events go back to the pool and before the next call reuses (or frees) the staging
    ~StagePipe() {
        (void)hipStreamSynchronize(c->stream);
        for (auto x : ev) if (x) c->evt_pool.push_back(x);
    }
    int ensure(size_t bytes_per_half) {  // the staging grows on demand and never shrinks
        per_half = bytes_per_half;
        if (2 * per_half <= c->stage_pinned_bytes) return 0;
        if (c->stage_pinned) (void)hipHostFree(c->stage_pinned);
        c->stage_pinned = nullptr; c->stage_pinned_bytes = 0;
        if (hipHostMalloc((void**)&c->stage_pinned, 2 * per_half, hipHostMallocDefault) != hipSuccess)
            return fail(-3, who + ": cannot page-lock " + std::to_string(2 * per_half) + " bytes");
        c->stage_pinned_bytes = 2 * per_half;
        return 0;
    }
    uint8_t* half(unsigned long long ci) const { return c->stage_pinned + (ci & 1) * per_half; }
    // queue(ci) launches chunk ci's kernels and queues its copy into half(ci); take(ci) finds the chunk there.  The first non-zero
    // return ends the loop.
    template <typename Queue, typename Take>
    int run(unsigned long long n_chunks, Queue queue, Take take) {
        auto wait_take = [&](unsigned long long ci) -> int {
            if (hipEventSynchronize(ev[ci & 1]) != hipSuccess) return fail(-2, who + ": " + lost);
            return take(ci);
        };
        for (unsigned long long ci = 0; ci < n_chunks; ci++) {
            CHECK(queue(ci));
            const hipError_t e = hipEventRecord(ev[ci & 1], c->stream);
            if (e != hipSuccess) return fail(-2, who + ": " + hipGetErrorString(e));
            if (ci) CHECK(wait_take(ci - 1));  // (chunk ci - 1's half of the staging is free again before chunk ci + 1 is queued)
        }
        return n_chunks ? wait_take(n_chunks - 1) : 0;
    }
};
