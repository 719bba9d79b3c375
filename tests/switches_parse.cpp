// The parse rules of csrc/fa_switches.h against a hand-written table: what every reader of the library as it was before that header
// (one lambda per site) answered for the unset case, each documented value, the lenient spellings it accepted and the number edge
// cases.  A stand-alone host program (tests/test_switches.py builds it under ASan + UBSan, with and without AULE_DEBUG_HOOKS).
// Every row is one fake environment of one variable; the expectation is the line aule_hip_debug_switches prints for that name, and
// every other line must be the default's.  Exit status 0 and "PARSE OK <rows>" when every row holds.
#include <cstdio>
#include <cstring>
#include <map>
#include <string>

#include "fa_switches.h"

namespace {

struct Row { const char* name; const char* text; const char* want; };   // text = nullptr: unset

#ifdef AULE_DEBUG_HOOKS
#define ONLY(word) word
#else
#define ONLY(word) "both"   // the product library launches both kernels whatever the variable says
#endif

const Row kRows[] = {
    // AULE_HIP_FWD_KERNEL: "pp" exactly; "w4" and "" are the default; any other text warned and ran the default dispatch
    {"AULE_HIP_FWD_KERNEL", nullptr, "default"}, {"AULE_HIP_FWD_KERNEL", "pp", "pp"}, {"AULE_HIP_FWD_KERNEL", "w4", "default"},
    {"AULE_HIP_FWD_KERNEL", "", "default"}, {"AULE_HIP_FWD_KERNEL", "ps", "default"}, {"AULE_HIP_FWD_KERNEL", "ppx", "default"},
    {"AULE_HIP_FWD_KERNEL", "p", "default"},
    // off only when the text starts with '0'
    {"AULE_HIP_FWD_SPLITKV", nullptr, "1"}, {"AULE_HIP_FWD_SPLITKV", "0", "0"}, {"AULE_HIP_FWD_SPLITKV", "1", "1"},
    {"AULE_HIP_FWD_SPLITKV", "00", "0"}, {"AULE_HIP_FWD_SPLITKV", "off", "1"}, {"AULE_HIP_FWD_SPLITKV", "", "1"},
    {"AULE_HIP_FWD_PPSPLIT", nullptr, "1"}, {"AULE_HIP_FWD_PPSPLIT", "0", "0"}, {"AULE_HIP_FWD_PPSPLIT", "1", "1"},
    {"AULE_HIP_FWD_PPSPLIT", "0x", "0"}, {"AULE_HIP_FWD_PPSPLIT", "no", "1"},
    // atoi when the text starts with a digit, at most 8; else 8
    {"AULE_HIP_FWD_SPLIT", nullptr, "8"}, {"AULE_HIP_FWD_SPLIT", "0", "0"}, {"AULE_HIP_FWD_SPLIT", "1", "1"}, {"AULE_HIP_FWD_SPLIT", "4", "4"},
    {"AULE_HIP_FWD_SPLIT", "8", "8"}, {"AULE_HIP_FWD_SPLIT", "99", "8"}, {"AULE_HIP_FWD_SPLIT", "-1", "8"}, {"AULE_HIP_FWD_SPLIT", "3x", "3"},
    {"AULE_HIP_FWD_SPLIT", "x", "8"}, {"AULE_HIP_FWD_SPLIT", "", "8"},
    // atoi when the text starts with a digit, else 16; at least 4
    {"AULE_HIP_FWD_SPLIT_MIN", nullptr, "16"}, {"AULE_HIP_FWD_SPLIT_MIN", "6", "6"}, {"AULE_HIP_FWD_SPLIT_MIN", "16", "16"},
    {"AULE_HIP_FWD_SPLIT_MIN", "40", "40"}, {"AULE_HIP_FWD_SPLIT_MIN", "0", "4"}, {"AULE_HIP_FWD_SPLIT_MIN", "3", "4"},
    {"AULE_HIP_FWD_SPLIT_MIN", "-5", "16"}, {"AULE_HIP_FWD_SPLIT_MIN", "9t", "9"}, {"AULE_HIP_FWD_SPLIT_MIN", "tiles", "16"},
    // first character
    {"AULE_HIP_FWD_SOFTMAX", nullptr, "default"}, {"AULE_HIP_FWD_SOFTMAX", "classic", "classic"}, {"AULE_HIP_FWD_SOFTMAX", "c", "classic"},
    {"AULE_HIP_FWD_SOFTMAX", "raw", "default"}, {"AULE_HIP_FWD_SOFTMAX", "Classic", "default"}, {"AULE_HIP_FWD_SOFTMAX", "", "default"},
    {"AULE_HIP_FWD_COMBINE", nullptr, "default"}, {"AULE_HIP_FWD_COMBINE", "wg", "wg"}, {"AULE_HIP_FWD_COMBINE", "w", "wg"},
    {"AULE_HIP_FWD_COMBINE", "rows", "default"}, {"AULE_HIP_FWD_COMBINE", "", "default"},
    {"AULE_HIP_W4_BODIES", nullptr, "default"}, {"AULE_HIP_W4_BODIES", "generic", "generic"}, {"AULE_HIP_W4_BODIES", "g", "generic"},
    {"AULE_HIP_W4_BODIES", "embedded", "default"}, {"AULE_HIP_W4_BODIES", "", "default"},
    {"AULE_HIP_W4_ORDER", nullptr, "default"}, {"AULE_HIP_W4_ORDER", "pairs", "pairs"}, {"AULE_HIP_W4_ORDER", "p", "pairs"},
    {"AULE_HIP_W4_ORDER", "rounds", "default"}, {"AULE_HIP_W4_ORDER", "", "default"},
    {"AULE_HIP_W4_UNPAIR", nullptr, "1"}, {"AULE_HIP_W4_UNPAIR", "0", "0"}, {"AULE_HIP_W4_UNPAIR", "1", "1"}, {"AULE_HIP_W4_UNPAIR", "off", "1"},
    {"AULE_HIP_W4_WINDOW", nullptr, "1"}, {"AULE_HIP_W4_WINDOW", "0", "0"}, {"AULE_HIP_W4_WINDOW", "1", "1"}, {"AULE_HIP_W4_WINDOW", "", "1"},
    // atoi only when the text starts with a digit, else 4
    {"AULE_HIP_W4_WTAIL", nullptr, "4"}, {"AULE_HIP_W4_WTAIL", "0", "0"}, {"AULE_HIP_W4_WTAIL", "4", "4"}, {"AULE_HIP_W4_WTAIL", "99", "99"},
    {"AULE_HIP_W4_WTAIL", "-1", "4"}, {"AULE_HIP_W4_WTAIL", "7x", "7"}, {"AULE_HIP_W4_WTAIL", "x7", "4"}, {"AULE_HIP_W4_WTAIL", "", "4"},
    // atof; negative (and text that is no number at all reads as 0) ...
    {"AULE_HIP_W4_SUMLO", nullptr, "default"}, {"AULE_HIP_W4_SUMLO", "0.5", "0.5"}, {"AULE_HIP_W4_SUMLO", "0.25", "0.25"},
    {"AULE_HIP_W4_SUMLO", "0", "0"}, {"AULE_HIP_W4_SUMLO", "-3", "default"}, {"AULE_HIP_W4_SUMLO", "-0.001", "default"},
    {"AULE_HIP_W4_SUMLO", "1e-3", "0.001"}, {"AULE_HIP_W4_SUMLO", "x", "0"}, {"AULE_HIP_W4_SUMLO", "nan", "default"},
    {"AULE_HIP_F32_SPLIT", nullptr, "1"}, {"AULE_HIP_F32_SPLIT", "0", "0"}, {"AULE_HIP_F32_SPLIT", "1", "1"}, {"AULE_HIP_F32_SPLIT", "false", "1"},
    // first character: r / s
    {"AULE_HIP_BWD_MODE", nullptr, "auto"}, {"AULE_HIP_BWD_MODE", "recompute", "recompute"}, {"AULE_HIP_BWD_MODE", "spill", "spill"},
    {"AULE_HIP_BWD_MODE", "auto", "auto"}, {"AULE_HIP_BWD_MODE", "random", "recompute"}, {"AULE_HIP_BWD_MODE", "s", "spill"},
    {"AULE_HIP_BWD_MODE", "Spill", "auto"}, {"AULE_HIP_BWD_MODE", "", "auto"},
    // atoll of any text; zero and below: 0 bytes
    {"AULE_HIP_BWD_DS_AUTO_MB", nullptr, "160"}, {"AULE_HIP_BWD_DS_AUTO_MB", "160", "160"}, {"AULE_HIP_BWD_DS_AUTO_MB", "1", "1"},
    {"AULE_HIP_BWD_DS_AUTO_MB", "0", "0"}, {"AULE_HIP_BWD_DS_AUTO_MB", "-5", "0"}, {"AULE_HIP_BWD_DS_AUTO_MB", "12x", "12"},
    {"AULE_HIP_BWD_DS_AUTO_MB", "x", "0"}, {"AULE_HIP_BWD_DS_AUTO_MB", "", "0"},
    {"AULE_HIP_BWD_DS_CAP_MB", nullptr, "8192"}, {"AULE_HIP_BWD_DS_CAP_MB", "2500", "2500"}, {"AULE_HIP_BWD_DS_CAP_MB", "500", "500"},
    {"AULE_HIP_BWD_DS_CAP_MB", "0", "0"}, {"AULE_HIP_BWD_DS_CAP_MB", "-1", "0"}, {"AULE_HIP_BWD_DS_CAP_MB", "100000", "100000"},
    // first character: o / n.  One field for both former readers: bwd_dkv4_applicable refused on 'o', bwd_dkv4_forced answered on 'n'
    {"AULE_HIP_BWD_DKV", nullptr, "default"}, {"AULE_HIP_BWD_DKV", "old", "old"}, {"AULE_HIP_BWD_DKV", "new", "new"},
    {"AULE_HIP_BWD_DKV", "o", "old"}, {"AULE_HIP_BWD_DKV", "never", "new"}, {"AULE_HIP_BWD_DKV", "default", "default"}, {"AULE_HIP_BWD_DKV", "", "default"},
    {"AULE_HIP_BWD_DQ", nullptr, "default"}, {"AULE_HIP_BWD_DQ", "old", "old"}, {"AULE_HIP_BWD_DQ", "new", "new"},
    {"AULE_HIP_BWD_DQ", "off", "old"}, {"AULE_HIP_BWD_DQ", "n", "new"}, {"AULE_HIP_BWD_DQ", "x", "default"},
    // '0' first: never; any other text, the empty one too: always
    {"AULE_HIP_BWD_DKV_K2", nullptr, "default"}, {"AULE_HIP_BWD_DKV_K2", "0", "0"}, {"AULE_HIP_BWD_DKV_K2", "1", "1"},
    {"AULE_HIP_BWD_DKV_K2", "2", "1"}, {"AULE_HIP_BWD_DKV_K2", "no", "1"}, {"AULE_HIP_BWD_DKV_K2", "", "1"}, {"AULE_HIP_BWD_DKV_K2", "01", "0"},
    // atoi of any text, non-zero: backwards
    {"AULE_HIP_DQS_REV", nullptr, "1"}, {"AULE_HIP_DQS_REV", "0", "0"}, {"AULE_HIP_DQS_REV", "1", "1"}, {"AULE_HIP_DQS_REV", "2", "1"},
    {"AULE_HIP_DQS_REV", "-1", "1"}, {"AULE_HIP_DQS_REV", "off", "0"}, {"AULE_HIP_DQS_REV", "", "0"},
    // the first two characters: w4 / dk
    {"AULE_TL", nullptr, "default"}, {"AULE_TL", "w4", "w4"}, {"AULE_TL", "dkv4", "dkv4"}, {"AULE_TL", "dk", "dkv4"}, {"AULE_TL", "w4x", "w4"},
    {"AULE_TL", "pp", "default"}, {"AULE_TL", "w", "default"}, {"AULE_TL", "d", "default"}, {"AULE_TL", "dq", "default"}, {"AULE_TL", "", "default"},
    {"AULE_TL_FLAGS", nullptr, "0"}, {"AULE_TL_FLAGS", "0", "0"}, {"AULE_TL_FLAGS", "3", "3"}, {"AULE_TL_FLAGS", "-2", "-2"},
    {"AULE_TL_FLAGS", "5x", "5"}, {"AULE_TL_FLAGS", "x", "0"},
    // the whole word, debug library only
    {"AULE_DBG_BWD_ONLY", nullptr, "both"}, {"AULE_DBG_BWD_ONLY", "dq", ONLY("dq")}, {"AULE_DBG_BWD_ONLY", "dkv", ONLY("dkv")},
    {"AULE_DBG_BWD_ONLY", "d", "both"}, {"AULE_DBG_BWD_ONLY", "dqx", "both"}, {"AULE_DBG_BWD_ONLY", "all", "both"}, {"AULE_DBG_BWD_ONLY", "", "both"},
    // '1' first
    {"AULE_ROCTX", nullptr, "0"}, {"AULE_ROCTX", "1", "1"}, {"AULE_ROCTX", "0", "0"}, {"AULE_ROCTX", "10", "1"}, {"AULE_ROCTX", "yes", "0"},
    {"AULE_ROCTX", "", "0"},
};

std::map<std::string, std::string> printed(const aule_hip::Switches& s) {
    char small[8];
    const uint64_t need = aule_hip::print_switches(s, small, sizeof small);   // a short buffer: truncated, NUL-terminated, the full size answered
    if (std::strlen(small) != sizeof small - 1 || need != aule_hip::print_switches(s, nullptr, 0)) std::abort();
    std::string text(need, '\0');
    if (aule_hip::print_switches(s, &text[0], need) != need) std::abort();
    text.resize(need - 1);
    std::map<std::string, std::string> m;
    for (size_t at = 0; at < text.size();) {
        const size_t nl = text.find('\n', at), eq = text.find('=', at);
        if (nl == std::string::npos || eq == std::string::npos || eq > nl) std::abort();
        m[text.substr(at, eq - at)] = text.substr(eq + 1, nl - eq - 1);
        at = nl + 1;
    }
    return m;
}

}  // namespace

int main() {
    const auto dflt = printed(aule_hip::read_switches([](const char*) -> const char* { return nullptr; }));
    int bad = 0, rows = 0;
    if (dflt.size() != 25) { std::printf("expected 25 switches, printed %zu\n", dflt.size()); ++bad; }
    if (printed(aule_hip::Switches{}) != dflt) { std::printf("the struct's initialisers are not the unset environment\n"); ++bad; }
    for (const Row& r : kRows) {
        ++rows;
        if (dflt.count(r.name) == 0) { std::printf("%s is not a switch\n", r.name); ++bad; continue; }
        const auto got = printed(aule_hip::read_switches([&r](const char* name) -> const char* { return std::strcmp(name, r.name) == 0 ? r.text : nullptr; }));
        for (const auto& kv : got) {
            const std::string want = kv.first == r.name ? r.want : dflt.at(kv.first);
            if (kv.second != want) {
                std::printf("%s=%s: %s reads %s, expected %s\n", r.name, r.text ? r.text : "(unset)", kv.first.c_str(), kv.second.c_str(), want.c_str());
                ++bad;
            }
        }
    }
    for (const auto& kv : dflt) {   // every switch has rows, its unset row among them
        int n = 0, unset = 0;
        for (const Row& r : kRows)
            if (kv.first == r.name) { ++n; unset += r.text == nullptr; }
        if (n < 4 || unset != 1) { std::printf("%s: %d rows, %d of them unset\n", kv.first.c_str(), n, unset); ++bad; }
    }
    // the values behind the printed words that a plan computes with
    {
        using namespace aule_hip;
        const auto env = [](const char* name) -> const char* {
            if (std::strcmp(name, "AULE_HIP_BWD_DS_CAP_MB") == 0) return "2500";
            if (std::strcmp(name, "AULE_HIP_BWD_DS_AUTO_MB") == 0) return "-7";
            if (std::strcmp(name, "AULE_HIP_BWD_DKV") == 0) return "new";
            if (std::strcmp(name, "AULE_HIP_W4_SUMLO") == 0) return "0.25";
            return nullptr;
        };
        const Switches s = read_switches(env);
        if (s.bwd_ds_cap_bytes != 2500ull << 20 || s.bwd_ds_auto_bytes != 0 || s.bwd_dkv != Pick::new_kernel || s.w4_sumlo != 0.25f ||
            Switches{}.bwd_ds_auto_bytes != 160ull << 20 || Switches{}.bwd_ds_cap_bytes != 8192ull << 20 || !(Switches{}.w4_sumlo < 0.f)) {
            std::printf("typed fields differ from their printed values\n");
            ++bad;
        }
    }
    if (bad) return 1;
    std::printf("PARSE OK %d\n", rows);
    return 0;
}
