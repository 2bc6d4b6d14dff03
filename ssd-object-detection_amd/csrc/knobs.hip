// Development overrides (ssd_dev_knob): A/B timing of kernel variants and forcing a dispatch path in tests, inside one
// process.  NOT configuration: the product never sets them, nothing is read from the environment, and results never
// depend on them (every variant computes the same convolution).  Values are relaxed atomics (KNOB_UNSET in the table:
// the caller's default applies), so concurrent calls are safe.  One table for the whole library: the convolution dispatch
// (conv.hip, conv_wgrad.hip, conv_common.h), match.hip, pwgemm.hip and sparse.hip read it through ssd_knob (common.h).
#include <atomic>
#include <climits>
#include <cstring>
#include "common.h"

namespace {

struct Knob { const char* name; std::atomic<int> value; };
constexpr int KNOB_UNSET = INT_MIN;
Knob g_knobs[] = {{"SSD_ABLATE", {KNOB_UNSET}}, {"SSD_DGRAD_S2", {KNOB_UNSET}},
                  {"SSD_CONV_PATCH", {KNOB_UNSET}}, {"SSD_CONV_TILE", {KNOB_UNSET}}, {"SSD_SPLITK", {KNOB_UNSET}},
                  {"SSD_WGRAD_PATCH", {KNOB_UNSET}},
                  {"SSD_WGRAD_PATCH_SHAPE", {KNOB_UNSET}}, {"SSD_WGRAD_TILE", {KNOB_UNSET}},
                  {"SSD_CONV_PATCH_FLAT", {KNOB_UNSET}}, {"SSD_WGRAD_FIRST", {KNOB_UNSET}}, {"SSD_CONV_FIRST", {KNOB_UNSET}},
                  {"SSD_WGRAD_PATCH_XCD", {KNOB_UNSET}}, {"SSD_CONV_C64", {KNOB_UNSET}}, {"SSD_CONV_POOL_FUSE", {KNOB_UNSET}},
                  {"SSD_CONV_PATCH_ROWFLAT", {KNOB_UNSET}}, {"SSD_MATCH_FUSED", {KNOB_UNSET}}, {"SSD_CONV_P512", {KNOB_UNSET}},
                  {"SSD_C64B_WGS", {KNOB_UNSET}}, {"SSD_CONV_PW", {KNOB_UNSET}}, {"SSD_PW_WGS", {KNOB_UNSET}},
                  {"SSD_SP_ABLATE", {KNOB_UNSET}}, {"SSD_EPI_PREFETCH", {KNOB_UNSET}}};
Knob* find_knob(const char* name) {
    for (Knob& k : g_knobs) if (!strcmp(k.name, name)) return &k;
    return nullptr;
}

}  // namespace

int ssd_knob(const char* name, int dflt) {
    Knob* k = find_knob(name);
    if (!k) return dflt;
    const int v = k->value.load(std::memory_order_relaxed);
    return v == KNOB_UNSET ? dflt : v;
}

extern "C" int ssd_dev_knob(const char* name, int value) {
    if (!name) return SSD_ERR_VALUE;
    Knob* k = find_knob(name);
    if (!k) return SSD_ERR_VALUE;
    k->value.store(value, std::memory_order_relaxed);
    return SSD_OK;
}
