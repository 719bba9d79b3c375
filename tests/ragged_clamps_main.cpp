// The clamp property of the ragged entries' memory-safety contract (include/aule.h), checked on the host: a stand-alone program over
// the helpers of csrc/fa_device.h, built with -fsanitize=address,undefined by tests/test_ragged_rules_host.py and run directly.
// Whatever cu[b], cu[b + 1] and ctx[b] hold: 0 <= s, 0 <= n <= cap, s + n <= T and 0 <= L <= cap -- and, without offsets (a null cu,
// sequence b owns row b < T), s = b and n = 1.  cu and ctx live in exactly sized heap arrays, so a read outside them is ASan's to report,
// and every sum is formed in int as the kernels form it, so an overflow is UBSan's.
#include <climits>
#include <cstdio>
#include <vector>

#include "fa_device.h"

int main() {
    using aule_hip::SeqRange;
    long cases = 0;
    for (int T : {0, 1, 7}) {
        const int hostile[8] = {INT_MIN, -1, 0, 1, T - 1, T, T + 1, INT_MAX};
        for (int cap : {1, 3, INT_MAX})
            for (int lo : hostile)
                for (int hi : hostile)
                    for (int len : hostile)
                        for (int b : {0, 1}) {   // (the arrays' first and last sequence)
                            std::vector<int> cu(3, 0), ctx(2, 0);
                            cu[b] = lo; cu[b + 1] = hi; ctx[b] = len;
                            const SeqRange r = aule_hip::seq_range(cu.data(), b, T, cap);
                            const SeqRange q = aule_hip::seq_range_or_row(cu.data(), b, T, cap);
                            const int L = aule_hip::seq_len(ctx.data(), b, cap);
                            const bool ok = r.s >= 0 && r.n >= 0 && r.n <= cap && (long long)r.s + r.n <= T && L >= 0 && L <= cap && q.s == r.s && q.n == r.n;
                            if (!ok) {
                                std::printf("FAILED: T %d cap %d cu[b] %d cu[b + 1] %d ctx[b] %d -> s %d n %d L %d\n", T, cap, lo, hi, len, r.s, r.n, L);
                                return 1;
                            }
                            ++cases;
                        }
    }
    // no offsets: sequence b owns row b, one token (cap >= 1)
    for (int b : {0, 5}) {
        const SeqRange r = aule_hip::seq_range_or_row(nullptr, b, 7, 3);
        if (r.s != b || r.n != 1) {
            std::printf("FAILED: null offsets, b %d -> s %d n %d\n", b, r.s, r.n);
            return 1;
        }
    }
    // the block lookup: the shift and the division agree
    for (int bs : {1, 16, 64})
        for (int j : {0, 1, 15, 16, 63, 64, 1000, (1 << 30) - 1})
            if (aule_hip::block_of(j, bs, __builtin_ctz((unsigned)bs)) != aule_hip::block_of(j, bs, -1)) {
                std::printf("FAILED: block_of(%d, %d)\n", j, bs);
                return 1;
            }
    std::printf("ok: %ld cases\n", cases);
    return 0;
}
