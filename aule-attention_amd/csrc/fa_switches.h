// fa_switches.h -- every run-time switch of the native library: one struct, one reader, one printer (host only, standard library only).
// The launch plans (fa_fwd_plan.h, fa_bwd_plan.h) and the launchers read fields of switches(); nothing else in csrc/ asks the environment
// (aule_init's AULE_BACKEND / AULE_HIP_DEVICE belong to the legacy handle API and are read on every call, in aule_capi.cpp).
// docs/SWITCHES.md has one row per name below; tests/test_switches.py holds the two together and pins every parse rule.
// The rules are lenient on purpose (mostly the first character decides): they are the rules the A/B scripts and tests were written against.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace aule_hip {

enum class FwdKernel { dflt, pp, unknown };     // unknown: a name that is no kernel of this build -- the default dispatch, after a warning
enum class BwdMode { automatic, recompute, spill };
enum class Pick { dflt, old_kernel, new_kernel };   // a one-wave-per-SIMD backward kernel: by the plan's grid rule / never / wherever it can run
enum class K2 { rule, never, always };
enum class Timeline { dflt, w4, dkv4 };
enum class BwdOnly { both, dq, dkv };

struct Switches {
    // forward
    FwdKernel fwd_kernel = FwdKernel::dflt;
    bool fwd_splitkv = true;            // route 4
    bool fwd_ppsplit = true;            // route 5
    int fwd_split = 8;                  // route 7: most pieces per pair of Q blocks (< 2: off) -- kMaxPieces of fa_fwd_split.h
    int fwd_split_min = 16;             // route 7: key tiles of the shortest piece -- kSplitMinTiles
    bool fwd_softmax_classic = false;
    bool fwd_combine_wg = false;
    bool w4_generic_bodies = false;
    bool w4_order_pairs = false;
    bool w4_unpair = true;
    bool w4_window = true;
    int w4_wtail = 4;
    float w4_sumlo = -1.0f;             // negative: the dtype's default bound (launch_w4)
    bool f32_split = true;
    // backward
    BwdMode bwd_mode = BwdMode::automatic;
    uint64_t bwd_ds_auto_bytes = 160ull << 20;
    uint64_t bwd_ds_cap_bytes = 8192ull << 20;
    Pick bwd_dkv = Pick::dflt;
    K2 bwd_dkv_k2 = K2::rule;
    Pick bwd_dq = Pick::dflt;
    bool dqs_rev = true;
    // debug
    Timeline tl = Timeline::dflt;
    int tl_flags = 0;
    BwdOnly dbg_bwd_only = BwdOnly::both;
    bool roctx = false;
};

namespace switch_rules {   // e: the variable's text, null when unset
inline bool starts(const char* e, char c) { return e != nullptr && e[0] == c; }
inline bool not_zero(const char* e) { return !starts(e, '0'); }                                // on unless the text starts with 0
inline int digits_or(const char* e, int dflt) { return (e != nullptr && e[0] >= '0' && e[0] <= '9') ? std::atoi(e) : dflt; }   // atoi of text that starts with a digit
inline int int_or(const char* e, int dflt) { return e != nullptr ? std::atoi(e) : dflt; }   // atoi of any text
inline Pick pick(const char* e) { return starts(e, 'o') ? Pick::old_kernel : (starts(e, 'n') ? Pick::new_kernel : Pick::dflt); }
inline uint64_t mb(const char* e, long long dflt) {   // a size in MB, as bytes; zero and below: 0
    const long long v = e != nullptr ? std::atoll(e) : dflt;
    return (uint64_t)(v > 0 ? v : 0) << 20;
}
inline FwdKernel fwd_kernel(const char* e) {
    if (e == nullptr || e[0] == 0 || std::strcmp(e, "w4") == 0) return FwdKernel::dflt;
    return std::strcmp(e, "pp") == 0 ? FwdKernel::pp : FwdKernel::unknown;
}
inline float sumlo(const char* e) {
    const float x = e != nullptr ? (float)std::atof(e) : -1.0f;
    return x >= 0.f ? x : -1.0f;
}
inline BwdMode bwd_mode(const char* e) { return starts(e, 'r') ? BwdMode::recompute : (starts(e, 's') ? BwdMode::spill : BwdMode::automatic); }
inline K2 k2(const char* e) { return e == nullptr ? K2::rule : (e[0] == '0' ? K2::never : K2::always); }
inline Timeline timeline(const char* e) {   // the first two characters
    return (starts(e, 'w') && e[1] == '4') ? Timeline::w4 : ((starts(e, 'd') && e[1] == 'k') ? Timeline::dkv4 : Timeline::dflt);
}
inline BwdOnly bwd_only(const char* e) {   // the whole word, and only in the debug library: the product launches both kernels whatever it says
#ifdef AULE_DEBUG_HOOKS
    if (e != nullptr) return std::strcmp(e, "dq") == 0 ? BwdOnly::dq : (std::strcmp(e, "dkv") == 0 ? BwdOnly::dkv : BwdOnly::both);
#endif
    (void)e;
    return BwdOnly::both;
}
}  // namespace switch_rules

// The switches of the environment `get` (name -> text, null when unset): a pure function, one line per switch -- name, rule, default.
template <class Lookup>
Switches read_switches(Lookup get) {
    using namespace switch_rules;
    Switches s;
    s.fwd_kernel = fwd_kernel(get("AULE_HIP_FWD_KERNEL"));                           // pp; w4 and "" are the default; anything else: unknown
    s.fwd_splitkv = not_zero(get("AULE_HIP_FWD_SPLITKV"));                            // on
    s.fwd_ppsplit = not_zero(get("AULE_HIP_FWD_PPSPLIT"));                            // on
    s.fwd_split = std::min(digits_or(get("AULE_HIP_FWD_SPLIT"), 8), 8);               // 8
    s.fwd_split_min = std::max(digits_or(get("AULE_HIP_FWD_SPLIT_MIN"), 16), 4);      // 16
    s.fwd_softmax_classic = starts(get("AULE_HIP_FWD_SOFTMAX"), 'c');                 // off
    s.fwd_combine_wg = starts(get("AULE_HIP_FWD_COMBINE"), 'w');                      // off
    s.w4_generic_bodies = starts(get("AULE_HIP_W4_BODIES"), 'g');                     // off
    s.w4_order_pairs = starts(get("AULE_HIP_W4_ORDER"), 'p');                         // off
    s.w4_unpair = not_zero(get("AULE_HIP_W4_UNPAIR"));                                // on
    s.w4_window = not_zero(get("AULE_HIP_W4_WINDOW"));                                // on
    s.w4_wtail = digits_or(get("AULE_HIP_W4_WTAIL"), 4);                              // 4
    s.w4_sumlo = sumlo(get("AULE_HIP_W4_SUMLO"));                                     // atof; negative, like unset: the dtype's default
    s.f32_split = not_zero(get("AULE_HIP_F32_SPLIT"));                                // on
    s.bwd_mode = bwd_mode(get("AULE_HIP_BWD_MODE"));                                  // r.. | s..; auto
    s.bwd_ds_auto_bytes = mb(get("AULE_HIP_BWD_DS_AUTO_MB"), 160);
    s.bwd_ds_cap_bytes = mb(get("AULE_HIP_BWD_DS_CAP_MB"), 8192);
    s.bwd_dkv = pick(get("AULE_HIP_BWD_DKV"));                                        // o.. | n..; the grid rule
    s.bwd_dkv_k2 = k2(get("AULE_HIP_BWD_DKV_K2"));                                    // 0.. never, any other text always; the whole-rounds rule
    s.bwd_dq = pick(get("AULE_HIP_BWD_DQ"));                                          // o.. | n..; the grid rule
    s.dqs_rev = int_or(get("AULE_HIP_DQS_REV"), 1) != 0;                      // atoi; on
    s.tl = timeline(get("AULE_TL"));                                                  // w4.. | dk..; the ping-pong / two-waves-per-SIMD timelines
    s.tl_flags = int_or(get("AULE_TL_FLAGS"), 0);                             // atoi; 0
    s.dbg_bwd_only = bwd_only(get("AULE_DBG_BWD_ONLY"));                              // dq | dkv; both
    s.roctx = starts(get("AULE_ROCTX"), '1');                                         // off
    return s;
}

// The process's switches, read from its environment on first use and never again.
inline const Switches& switches() {
    static const Switches s = [] {
        const auto get = [](const char* name) -> const char* { return std::getenv(name); };
        const Switches r = read_switches(get);
        // ("ps" named the persistent tile stream retired in round 4 and used to be ignored silently: an A/B run then
        // measured the default kernel twice)
        if (r.fwd_kernel == FwdKernel::unknown)
            fprintf(stderr, "libaule: WARNING: AULE_HIP_FWD_KERNEL=%s is not a kernel of this build (known: pp, w4) -- the default dispatch runs\n",
                    get("AULE_HIP_FWD_KERNEL"));
        return r;
    }();
    return s;
}

// `s` as text, one line per switch in the order of read_switches: NAME=<resolved value>\n, the unset default spelt like any other value
// (aule_hip_debug_switches).  Writes at most cap bytes, NUL included; returns the bytes the whole text needs, NUL included.
inline uint64_t print_switches(const Switches& s, char* buf, uint64_t cap) {
    const auto pick = [](Pick p) { return p == Pick::old_kernel ? "old" : (p == Pick::new_kernel ? "new" : "default"); };
    char sumlo[32];
    if (s.w4_sumlo >= 0.f) std::snprintf(sumlo, sizeof sumlo, "%g", (double)s.w4_sumlo);
    else std::snprintf(sumlo, sizeof sumlo, "default");
    const int n = std::snprintf(
        buf, cap > 0 && buf != nullptr ? (size_t)cap : 0,
        "AULE_HIP_FWD_KERNEL=%s\nAULE_HIP_FWD_SPLITKV=%d\nAULE_HIP_FWD_PPSPLIT=%d\nAULE_HIP_FWD_SPLIT=%d\nAULE_HIP_FWD_SPLIT_MIN=%d\n"
        "AULE_HIP_FWD_SOFTMAX=%s\nAULE_HIP_FWD_COMBINE=%s\nAULE_HIP_W4_BODIES=%s\nAULE_HIP_W4_ORDER=%s\nAULE_HIP_W4_UNPAIR=%d\n"
        "AULE_HIP_W4_WINDOW=%d\nAULE_HIP_W4_WTAIL=%d\nAULE_HIP_W4_SUMLO=%s\nAULE_HIP_F32_SPLIT=%d\n"
        "AULE_HIP_BWD_MODE=%s\nAULE_HIP_BWD_DS_AUTO_MB=%llu\nAULE_HIP_BWD_DS_CAP_MB=%llu\nAULE_HIP_BWD_DKV=%s\nAULE_HIP_BWD_DKV_K2=%s\n"
        "AULE_HIP_BWD_DQ=%s\nAULE_HIP_DQS_REV=%d\nAULE_TL=%s\nAULE_TL_FLAGS=%d\nAULE_DBG_BWD_ONLY=%s\nAULE_ROCTX=%d\n",
        s.fwd_kernel == FwdKernel::pp ? "pp" : "default", (int)s.fwd_splitkv, (int)s.fwd_ppsplit, s.fwd_split, s.fwd_split_min,
        s.fwd_softmax_classic ? "classic" : "default", s.fwd_combine_wg ? "wg" : "default", s.w4_generic_bodies ? "generic" : "default",
        s.w4_order_pairs ? "pairs" : "default", (int)s.w4_unpair, (int)s.w4_window, s.w4_wtail, sumlo, (int)s.f32_split,
        s.bwd_mode == BwdMode::recompute ? "recompute" : (s.bwd_mode == BwdMode::spill ? "spill" : "auto"),
        (unsigned long long)(s.bwd_ds_auto_bytes >> 20), (unsigned long long)(s.bwd_ds_cap_bytes >> 20), pick(s.bwd_dkv),
        s.bwd_dkv_k2 == K2::never ? "0" : (s.bwd_dkv_k2 == K2::always ? "1" : "default"), pick(s.bwd_dq), (int)s.dqs_rev,
        s.tl == Timeline::w4 ? "w4" : (s.tl == Timeline::dkv4 ? "dkv4" : "default"), s.tl_flags,
        s.dbg_bwd_only == BwdOnly::dq ? "dq" : (s.dbg_bwd_only == BwdOnly::dkv ? "dkv" : "both"), (int)s.roctx);
    return n < 0 ? 0 : (uint64_t)n + 1;
}

}  // namespace aule_hip
