// fa_fwd_splitkv_body.inc -- the body of fa_fwd_splitkv_kernel, fa_fwd_paged_query_kernel and fa_fwd_paged_tree_kernel
// (fa_fwd_splitkv_gfx950.hip, which says why it is an include).  In scope: T, D, KV, the constants PAGED, MQ and TREE, and the kernel
// argument `const SplitParams p`.
    static_assert(PAGED || !MQ, "the multi-query instances are paged");
    static_assert(MQ || !TREE, "the tree instances are multi-query");
    using v8 = typename T::v8;
    constexpr int EB = KV::EB;
    constexpr int RB = D * EB;            // bytes of a K/V row
    constexpr int KS = D / 16, DB = D / 32;
    constexpr int NL = RB / 32;           // 16-byte loads per lane and tile, of K (a row over the two lane halves) and of V (32 rows over 64 lanes)
    constexpr int VT = 32 * D * 2;        // one wave's V tile in LDS (16-bit)
    __shared__ __attribute__((aligned(16))) char smem[4 * VT];

    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    char* const Vw = smem + wave * VT;

    const int g = p.Hq / p.Hkv;
    const int unit = blockIdx.y / p.nrt, rt = blockIdx.y % p.nrt;
    const int b = unit / p.Hkv, hk = unit % p.Hkv;
    const int Sq = (PAGED && !MQ) ? 1 : p.Sq;      // paged decode: one query token per sequence
    // paged: keys of this sequence, read on the device and bounded by what the block table can address (a stale or
    // corrupt scheduler value must not index the table or the cache out of bounds)
    const int Sk = PAGED ? min(max(p.context_lens[b], 0), p.max_blocks * p.block_size) : p.Sk;
    const int row = rt * 32 + l31;                 // packed row of this lane inside the unit
    const bool valid = row < g * Sq;
    const int head = hk * g + (valid ? row / Sq : 0), qi = valid ? row % Sq : 0;
    // MQ: position of this lane's query, and the smallest / largest position among the rows of this 32-row tile (wave-uniform:
    // a tile inside one head holds a range of queries, a tile across a head boundary holds query 0 and query Sq - 1)
    const int pos = MQ ? Sk - Sq + qi : 0;
    int pos_lo = 0, pos_hi = 0;
    if constexpr (MQ) {
        const int r0 = rt * 32, r1 = min(r0 + 31, g * Sq - 1);
        const bool one_head = r0 / Sq == r1 / Sq;
        pos_lo = Sk - Sq + (one_head ? r0 % Sq : 0);
        pos_hi = Sk - Sq + (one_head ? r1 % Sq : Sq - 1);
    }
    // TREE: the row's word, bit t = new token t (key Sk - Sq + t) is visible; as two halves, so that the test in the loop is a select and
    // a 32-bit shift.  A row at a negative position sees nothing (it has no context key either: Sk < Sq)
    unsigned tree_lo = 0u, tree_hi = 0u;
    if constexpr (TREE) {
        if (valid && pos >= 0) {
            const unsigned long long w = (unsigned long long)p.tree_mask[(size_t)b * Sq + qi];
            tree_lo = (unsigned)w;
            tree_hi = (unsigned)(w >> 32);
        }
    }

    const size_t kvoff = PAGED ? 0 : (size_t)(b * p.Hkv + hk) * Sk * RB;
    const __amdgpu_buffer_rsrc_t krs = skv_srd(reinterpret_cast<const char*>(p.k) + kvoff, PAGED ? 0u : (unsigned)Sk * RB);
    const __amdgpu_buffer_rsrc_t vrs = skv_srd(reinterpret_cast<const char*>(p.v) + kvoff, PAGED ? 0u : (unsigned)Sk * RB);
    // paged: byte address of key/value row `kv` of this unit inside the cache (64-bit: caches exceed 4 GiB)
    const int* const bt = PAGED ? p.block_tables + (size_t)b * p.max_blocks : nullptr;
    auto paged_row = [&](int kv) -> size_t {
        const int lb = kv / p.block_size, off = kv - lb * p.block_size;
        const size_t phys = (size_t)bt[min(lb, p.max_blocks - 1)];   // (tiles are rounded up: rows past Sk are masked, never out of the table)
        return ((phys * p.block_size + off) * p.Hkv + hk) * (size_t)RB;
    };

    // Q fragments (B operand of S^T = K.Q^T): fragment ks of lane (row, hi) holds d = KV::q_d0(ks, hi) .. +7, the k order
    // of the source's K operands; rows beyond the unit are 0
    v8 qf[KS];
    {
        const char* qrow = reinterpret_cast<const char*>(p.q) + ((size_t)(b * p.Hq + head) * Sq + qi) * (D * 2);
        const unsigned flip = (KV::kSignInQ && p.negq) ? 0x80008000u : 0u;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            u32x4_t x = {0u, 0u, 0u, 0u};
            if (valid) x = *reinterpret_cast<const u32x4_t*>(qrow + KV::q_d0(ks, hi) * 2);
            x[0] ^= flip; x[1] ^= flip; x[2] ^= flip; x[3] ^= flip;
            qf[ks] = as_v8<T>(x);
        }
    }

    // V staging map: the wave's 16-byte source chunks u = lane + 64 i fill the sub-tiled 16-bit image linearly
    // ([kv/4][d/16][4][16 elements]: fa_fwd_pp_gfx950.hip); a sub-tile row of 16 elements is EB source chunks, and chunk
    // u lands at byte u * 32 / EB of the image.  Transpose-read offset: fa_fwd_pp_gfx950.hip
    int v_g[NL], v_row[NL], v_col[NL];
#pragma unroll
    for (int i = 0; i < NL; ++i) {
        const int u = lane + 64 * i;
        const int bidx = u / (4 * EB);    // sub-tile index = kv4 * (D/16) + d16
        v_row[i] = (bidx / (D / 16)) * 4 + ((u / EB) & 3);
        v_col[i] = ((bidx % (D / 16)) * EB + u % EB) * 16;   // byte offset inside the row
        v_g[i] = v_row[i] * RB + v_col[i];
    }
    const int tr_off = hi * (D / 16) * 128 + ((lane >> 4) & 1) * 128 + (lane & 15) * 8;
    // paged fast path (power-of-two block size >= 8): block index inside the tile and byte offset inside the block
    const bool pow2 = PAGED && p.block_size >= 8 && (p.block_size & (p.block_size - 1)) == 0;
    const int bs_log2 = PAGED ? 31 - __builtin_clz(p.block_size | 1) : 0;
    const size_t blk_bytes = PAGED ? (size_t)p.block_size * p.Hkv * RB : 0;
    int k_jb = 0, k_off = 0, v_jb[NL], v_off[NL];
#pragma unroll
    for (int i = 0; i < NL; ++i) { v_jb[i] = 0; v_off[i] = 0; }
    if (pow2) {
        k_jb = l31 >> bs_log2;
        k_off = ((l31 & (p.block_size - 1)) * p.Hkv + hk) * RB + hi * 16;
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            v_jb[i] = v_row[i] >> bs_log2;
            v_off[i] = ((v_row[i] & (p.block_size - 1)) * p.Hkv + hk) * RB + v_col[i];
        }
    }

    f32x16_t o[DB];
#pragma unroll
    for (int d = 0; d < DB; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[d][r] = 0.f;
    float m = -INFINITY, l = 0.f;
    const float c = p.c * KV::k_factor(p, hk);   // (FP8: logits = k_scale * (q . codes) * scale, one fp32 factor per unit)

    const int ntiles = (Sk + 31) / 32;
    int t0 = (blockIdx.x * 4 + wave) * p.chunk_tiles;
    int t1 = min(t0 + p.chunk_tiles, ntiles);
    if constexpr (TREE) {
        // every tile below Sk: a node may see a new token behind its own position; no window over a tree
    } else if constexpr (MQ) {
        if (p.window > 0) t0 = max(t0, max(0, pos_lo - p.window + 1) / 32);   // tiles entirely before the window of every row
        t1 = min(t1, pos_hi < 0 ? 0 : pos_hi / 32 + 1);                       // tiles entirely behind the last row's position
    } else if constexpr (PAGED) {
        if (p.window > 0) t0 = max(t0, max(0, Sk - p.window) / 32);   // tiles entirely before the window
    }
    f32x16_t z;
#pragma unroll
    for (int r = 0; r < 16; ++r) z[r] = 0.f;

    for (int t = t0; t < t1; ++t) {
        const int kv0 = t * 32;
        // lane (key l31, hi) loads the 16-byte chunks 2j + hi of its K row; V chunk i of the staging map
        u32x4_t kx[NL], vx[NL];
        if constexpr (PAGED) {
            const u32x4_t zero = {0u, 0u, 0u, 0u};
            const bool kin = kv0 + l31 < Sk;
            if (pow2) {
                // power-of-two block sizes >= 8 (the usual 16/32/64/128): the tile's <= 4 logical blocks are looked up
                // ONCE per tile with wave-uniform (scalar) loads; each lane picks its block with selects and adds a
                // 32-bit in-block offset computed once per launch -- no per-lane table lookups or 64-bit multiplies
                const int lb0 = kv0 >> bs_log2;
                const size_t tile_off = (size_t)(kv0 & (p.block_size - 1)) * p.Hkv * RB;   // blocks larger than a tile
                // (four named values, not an array: the compiler turns selects over an array into an indexed read from scratch)
                const size_t pb0 = (size_t)bt[min(lb0, p.max_blocks - 1)] * blk_bytes + tile_off;
                const size_t pb1 = (size_t)bt[min(lb0 + 1, p.max_blocks - 1)] * blk_bytes + tile_off;
                const size_t pb2 = (size_t)bt[min(lb0 + 2, p.max_blocks - 1)] * blk_bytes + tile_off;
                const size_t pb3 = (size_t)bt[min(lb0 + 3, p.max_blocks - 1)] * blk_bytes + tile_off;
                auto pick = [&](int jb) -> size_t { return jb == 0 ? pb0 : (jb == 1 ? pb1 : (jb == 2 ? pb2 : pb3)); };
                const char* krow = reinterpret_cast<const char*>(p.k) + pick(k_jb) + k_off;
#pragma unroll
                for (int j = 0; j < NL; ++j) kx[j] = kin ? *reinterpret_cast<const u32x4_t*>(krow + j * 32) : zero;
#pragma unroll
                for (int i = 0; i < NL; ++i) {
                    const bool vin = kv0 + v_row[i] < Sk;
                    vx[i] = vin ? *reinterpret_cast<const u32x4_t*>(reinterpret_cast<const char*>(p.v) + pick(v_jb[i]) + v_off[i]) : zero;
                }
            } else {
                const char* krow = reinterpret_cast<const char*>(p.k) + (kin ? paged_row(kv0 + l31) : 0) + hi * 16;
#pragma unroll
                for (int j = 0; j < NL; ++j) kx[j] = kin ? *reinterpret_cast<const u32x4_t*>(krow + j * 32) : zero;
#pragma unroll
                for (int i = 0; i < NL; ++i) {
                    const bool vin = kv0 + v_row[i] < Sk;
                    vx[i] = vin ? *reinterpret_cast<const u32x4_t*>(reinterpret_cast<const char*>(p.v) + paged_row(kv0 + v_row[i]) + v_col[i]) : zero;
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < NL; ++j)
                kx[j] = __builtin_amdgcn_raw_buffer_load_b128(krs, (kv0 + l31) * RB + (2 * j + hi) * 16, 0, 0);
#pragma unroll
            for (int i = 0; i < NL; ++i) vx[i] = __builtin_amdgcn_raw_buffer_load_b128(vrs, v_g[i], kv0 * RB, 0);
        }
        f32x16_t s;
#pragma unroll
        for (int j = 0; j < NL; ++j) s = KV::template qk<T>(kx[j], &qf[j * (2 / EB)], j == 0 ? z : s);   // (2 / EB fragments per load)
#pragma unroll
        for (int i = 0; i < NL; ++i) KV::template stage_v<T>(Vw + (lane + 64 * i) * (32 / EB), vx[i]);

        // online softmax over this tile's 32 keys (16 per lane half), exp2 domain
        // (MQ: some row of the tile has a key behind its position -- the tile reaches past pos_lo -- or in front of its window)
        // (TREE: the tile reaches the new tokens)
        const bool ragged = TREE ? kv0 + 31 >= Sk - Sq
                          : MQ ? (kv0 + 31 > pos_lo || (p.window > 0 && pos_hi - kv0 >= p.window))
                          : (kv0 + 32 > Sk || (PAGED && p.window > 0 && Sk - 1 - kv0 >= p.window));
        float mx = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float x = s[r] * c;
            if (ragged) {
                const int kv = kv0 + crow(r, hi);
                if constexpr (TREE) {
                    const int bit = kv - (Sk - Sq);   // of the word: a new token (bit >= 0) is visible iff it lies below Sk and its bit is set
                    const unsigned half = (bit & 32) ? tree_hi : tree_lo;
                    if (bit >= 0 && (kv >= Sk || ((half >> (bit & 31)) & 1u) == 0u)) x = -INFINITY;
                } else if constexpr (MQ) {
                    if (kv > pos || (p.window > 0 && pos - kv >= p.window)) x = -INFINITY;   // (pos < Sk: keys past Sk included)
                } else {
                    if (kv >= Sk || (PAGED && p.window > 0 && Sk - 1 - kv >= p.window)) x = -INFINITY;
                }
            }
            s[r] = x;
            mx = fmaxf(mx, x);
        }
        mx = fmaxf(mx, xhalf(mx));
        const float m_new = fmaxf(m, mx);   // finite: every tile has at least one key < Sk (MQ: not so)
        // MQ: a row may have seen no key yet, this tile included.  Its m stays -inf and its exponentials are taken against 0, not
        // against -inf (-inf - -inf is a NaN): alpha and every p are exp2(-inf) = 0, so l and O stay 0
        const float m_ref = (MQ && m_new == -INFINITY) ? 0.f : m_new;
        const float alpha = fast_exp2(m - m_ref);
        m = m_new;
        float ls = 0.f;
        u32x4_t pu[2];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float p0 = fast_exp2(s[2 * i] - m_ref), p1 = fast_exp2(s[2 * i + 1] - m_ref);
            ls += p0 + p1;
            pu[i >> 2][i & 3] = T::pack2(p0, p1);
        }
        l = l * alpha + ls;
#pragma unroll
        for (int d = 0; d < DB; ++d)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[d][r] *= alpha;
        // O^T += V^T . P^T  (A by transpose read from the wave's LDS tile; k-slot order = S accumulator order)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int d = 0; d < DB; ++d) {
                const int off = ((4 * kk) * (D / 16) + 2 * d) * 128;
                const s16x4_t a0 = lds_tr16(Vw + tr_off + off);
                const s16x4_t a1 = lds_tr16(Vw + tr_off + off + 2 * (D / 16) * 128);
                o[d] = T::mfma(as_v8<T>(a0, a1), as_v8<T>(pu[kk]), o[d]);
            }
    }

    // partial of this wave: O (un-normalised, times the source's V factor), m, l of the lane's row (both lane halves
    // hold the same row)
    const float vs = KV::v_factor(p, hk);
    const float lt = l + xhalf(l);
    const int pi = blockIdx.x * 4 + wave;
    const size_t prow = (size_t)pi * p.rows_total + (size_t)blockIdx.y * 32 + l31;
    float* dst = p.part + prow * (D + 2);
#pragma unroll
    for (int d = 0; d < DB; ++d)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const f32x4_t x = {o[d][4 * g4] * vs, o[d][4 * g4 + 1] * vs, o[d][4 * g4 + 2] * vs, o[d][4 * g4 + 3] * vs};
            *reinterpret_cast<f32x4_t*>(dst + 32 * d + 8 * g4 + 4 * hi) = x;
        }
    if (hi == 0) {
        dst[D] = m;
        dst[D + 1] = lt;
    }
