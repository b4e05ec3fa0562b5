// The tune knobs' storage and their three entry points (tune.h holds the table).  Host code only.
#include "vz_common.h"

#include "tune.h"

namespace {

struct KnobInfo { int knob; const char* name; int dflt, lo, hi; };
const KnobInfo k_knobs[] = {
#define X(num, id, name, dflt, lo, hi, doc) {num, #name, dflt, lo, hi},
    VZ_KNOBS(X)
#undef X
};
const KnobInfo* find_knob(int knob) {
    for (const auto& k : k_knobs) if (k.knob == knob) return &k;
    return nullptr;
}
constexpr VzKnobValues knob_defaults() {
    VzKnobValues d{};
#define X(num, id, name, dflt, lo, hi, doc) d.v[num] = dflt;
    VZ_KNOBS(X)
#undef X
    return d;
}
unsigned g_tune_epoch = 0;

}  // namespace

VzKnobValues g_vz_knobs = knob_defaults();
unsigned vz_tune_epoch() { return g_tune_epoch; }

extern "C" int vz_tune_set(int knob, int value) {
    const KnobInfo* k = find_knob(knob);
    VZ_CHECK_ARG(k, "tune_set: unknown knob %d", knob);
    if (knob == VZ_KNOB_SPLITK_CAP) value = value < k->lo ? k->lo : (value > k->hi ? k->hi : value);       // the one knob that clamps (tune.h)
    VZ_CHECK_ARG(value >= k->lo && value <= k->hi, "tune_set: knob %d (%s) takes %d..%d, not %d", knob, k->name, k->lo, k->hi, value);
    g_vz_knobs.v[knob] = value;
    ++g_tune_epoch;          // also when the value is unchanged: the next vz_llm_decode_steps captures again
    return VZ_OK;
}

extern "C" int vz_tune_get(int knob, int* value) {
    VZ_CHECK_ARG(value && find_knob(knob), "tune_get: unknown knob %d or null argument", knob);
    *value = g_vz_knobs.v[knob];
    return VZ_OK;
}

extern "C" int vz_tune_info(int index, int* knob, const char** name, int* dflt, int* lo, int* hi) {
    VZ_CHECK_ARG(index >= 0 && index < (int)(sizeof(k_knobs) / sizeof(k_knobs[0])) && knob && name && dflt && lo && hi, "tune_info: no entry %d, or a null argument", index);
    const KnobInfo& k = k_knobs[index];
    *knob = k.knob; *name = k.name; *dflt = k.dflt; *lo = k.lo; *hi = k.hi;
    return VZ_OK;
}
