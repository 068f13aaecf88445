// Timing probe: hipEvents recorded around each launch on the caller's stream (GmcProbeScope, gmc_common.h), read back
// by gmc_probe_end / gmc_probe_flavours.  Off by default (no events, capture-safe).
#include "gmc_common.h"
#include <vector>

namespace {
struct ProbeRec { int tag; int flv; hipEvent_t a, b; };
struct ProbeState {
    bool on = false;
    std::vector<ProbeRec> pool;
    size_t used = 0;
} g_probe;
}  // namespace

void gmc_probe_mark(int tag, bool begin, hipStream_t st) {
    if (!g_probe.on) return;
    if (begin) {
        if (g_probe.used >= g_probe.pool.size()) return;  // capacity exhausted: stop recording
        ProbeRec &r = g_probe.pool[g_probe.used];
        r.tag = tag;
        r.flv = 0;
        (void)hipEventRecord(r.a, st);
    } else {
        if (g_probe.used >= g_probe.pool.size()) return;
        ProbeRec &r = g_probe.pool[g_probe.used];
        if (r.tag != tag) return;
        (void)hipEventRecord(r.b, st);
        ++g_probe.used;
    }
}

void gmc_probe_flavour(int word) {
    if (g_probe.on && g_probe.used < g_probe.pool.size()) g_probe.pool[g_probe.used].flv = word;   // (the open record)
}

extern "C" int gmc_probe_begin(int32_t capacity) {
    if (capacity < 0) return GMC_ERR_SHAPE;
    while ((int)g_probe.pool.size() < capacity) {
        ProbeRec r{-1, 0, nullptr, nullptr};
        hipError_t e = hipEventCreate(&r.a);
        if (e == hipSuccess) e = hipEventCreate(&r.b);
        if (e != hipSuccess) return (int)e;
        g_probe.pool.push_back(r);
    }
    g_probe.used = 0;
    g_probe.on = capacity > 0;
    return GMC_OK;
}

extern "C" int gmc_probe_end(int32_t *tags, float *ms, int32_t max) {
    g_probe.on = false;
    const int n = (int)g_probe.used;
    if (n > 0) {
        hipError_t e = hipEventSynchronize(g_probe.pool[n - 1].b);
        if (e != hipSuccess) return -(int)e - 1000;
    }
    for (int i = 0; i < n && i < max; ++i) {
        float t = 0.f;
        (void)hipEventElapsedTime(&t, g_probe.pool[i].a, g_probe.pool[i].b);
        if (tags) tags[i] = g_probe.pool[i].tag;
        if (ms) ms[i] = t;
    }
    return n;
}

extern "C" int gmc_probe_flavours(int32_t *words, int32_t max) {
    if (g_probe.on) return GMC_ERR_UNSUPPORTED;   // (after gmc_probe_end)
    const int n = (int)g_probe.used;
    for (int i = 0; i < n && i < max; ++i)
        if (words) words[i] = g_probe.pool[i].flv;
    return n;
}
