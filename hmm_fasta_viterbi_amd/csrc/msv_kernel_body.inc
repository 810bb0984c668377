// msv_kernel_body.inc -- the body of one launch over one profile's batch, included by msv_batch_kernel
// (MSV_BLOCK = blockIdx.x, MSV_BLOCKS = gridDim.x) and by msv_grid_kernel (the workgroup's index and
// count within its profile's share of the grid).  In scope: template parameters G, S, WAVES, PF, BIG,
// D, SA, RPFO and the launch's arguments `a` (msv_kernel.hip).
    constexpr bool SPLIT = SA > 0;
    // WIDE: the zero-copy twin of a residue-block variant (see BLK below and zc_fn, msv_kernel_impl.h).
    constexpr bool WIDE = RPFO == kWideBlocks;
    constexpr bool CLOCK = RPFO == kClockTwin;  // diagnostic twin: stamps also record s_memtime (bench clock_GHz)
    constexpr int SW = CLOCK ? kStampWords : 4;  // stamp words per wave (4 in the production kernels)
    // SPLIT needs the next row's residue one row early (B-chunk prefetch): at least 2 rows.
    constexpr int RPF0 = (RPFO > 0 && !WIDE) ? RPFO : residue_prefetch<S>();
    using St = Stream<S, (SPLIT && RPF0 < 2) ? 2 : RPF0>;
    static_assert(SPLIT ? (S - SA) % 2 == 0 : S % 4 == 0, "float4 chunks (A block), float2 halves (B block)");
    static_assert(PF >= 1 && D >= 1 && D <= 2, "PF >= 1, D in {1, 2}");
    static_assert(!SPLIT || (G >= 32 && !BIG && D == 1 && SA % 4 == 0 && SA < S), "split: 32/64-lane groups");
    constexpr int C4 = S / 4;
    constexpr int CA = SPLIT ? SA / 4 : C4;  // float4 chunks per lane whose emissions are staged in LDS
    constexpr int HB = SPLIT ? (S - SA) / 2 : 0;  // SPLIT: float2 halves per lane read from the B table
    constexpr int ROW_F4 = CA * G;           // float4 per LDS residue row
    constexpr int HBP = (HB + 1) & ~1;       // SPLIT: halves per lane in the B table (padded to even)
    constexpr int LDS_ROWS = SPLIT ? kAminoAcids : lds_rows_for(G, S);
    // Residue slots rotate instead of shifting (ROT): the row of phase P reads its residue from
    // r[P] and loads the residue RPF rows ahead into the same slot, and the main loop is unrolled
    // over the RPF phases.  A shift register moves every prefetched byte once per row, and a move of
    // a register with a load in flight waits for that load (s_waitcnt vmcnt(0) in every row): the
    // short rows of small profiles then last as long as one L2 round trip.  Paths that keep the
    // shift: one residue of prefetch (nothing to shift), the G = 64 row-class layout and D = 2.
    constexpr bool ROT = !BIG && D == 1 && St::RPF > 1;
    // Residue BLOCKS (BLK, short rows with G >= 16): instead of one byte load per row, every lane
    // loads one byte of a 16-row block (lane b of each DPP row: the row of phase b), once per 16
    // rows, a block ahead; a row takes its residue with one row_newbcast DPP move.  The row loop is
    // unrolled over the 16 phases and the block in flight is consumed 14-16 rows after its load, so
    // the waits the compiler places at the loop header or after a rare path (which merge every load
    // in flight: with per-row slots the header waited for the load of the row before, once per RPF
    // rows -- the bound of cfg2's 100.hmm rows) find it landed.  16x fewer VMEM instructions.
    // rows per block: 16 for short rows; none for long rows (one residue of prefetch): 8- or 16-row
    // blocks there saved ~2 VALU per row but unrolled 2-4k instructions per loop, cfg3 +0.7% / +3.5%
    // (profiles/r02_ab_blocks_long_rows.jsonl)
    constexpr int BLKN = St::RPF > 1 ? 16 : 0;
    constexpr bool BLK = !BIG && D == 1 && G >= 16 && !SPLIT && BLKN > 0;
    // WIDE blocks (residues in page-locked host memory, read over PCIe): a 16-lane group's byte loads
    // are 16-byte requests, and cfg2's 4 MB then crossed PCIe as 250k small completions (kernel 170 us
    // vs 96 us from HBM, profiles/r03_cfg2_host_call_timeline.txt).  The twin loads SUPERBLOCKS of
    // 64 rows instead -- lane b of each DPP row one (unaligned) dword, rows 4b .. 4b+3 -- two
    // superblocks ahead of use (a current and a next one), and derives each 16-row block from the
    // current superblock with one ds_bpermute (row 16k + b sits in lane 4k + b/4, byte b % 4) and a
    // byte extract, once per 16 rows: 64-byte requests, 4x fewer.
    static_assert(!WIDE || BLK, "wide blocks are the zero-copy form of residue blocks");
    constexpr int NPH = BLK ? BLKN : St::RPF;  // phases of the unrolled row loop
    // Cross-row emission prefetch: when the ring holds a whole row (small profiles), the NEXT row's
    // chunks are requested right after this row's last cell update, so the LDS latency hides behind
    // the E butterfly and the specials instead of stalling the start of every row.
    constexpr bool XROW = !BIG && !SPLIT && D == 1 && PF >= C4 && St::RPF >= 2;
    // ... and two rows ahead when the residue slots rotate over an even number of phases: rows of
    // even and odd phase keep their own ring, refilled with the row after next right after use, so
    // the LDS reads have a whole row to land instead of the epilogue's dozen instructions (cfg2:
    // 100.hmm rows are ~35 VALU, and waves spent 67% of their cycles in s_waitcnt, PMC r02).
    constexpr bool XROW2 = XROW && NPH % 2 == 0 && PF <= 2;  // +4 PF VGPRs
    static_assert(SPLIT || BIG == (LDS_ROWS < kTableRows), "BIG <=> table does not fit LDS");
    // LAZY rows (hand-ordered long rows at 4 waves per SIMD: msv_kernel.h lazy_e_rows) skip the E maximum of a
    // row on which no lane of the wave can raise its group's J (see `row`).  The per-lane bound table
    // [21][G] floats follows the emission table in a.etab and in LDS.
    constexpr bool LAZY = lazy_e_rows(S, WAVES, PF, BIG, SA, D);
    constexpr int EMAX_F4 = LAZY ? kTableRows * G / 4 : 0;
    static_assert((LDS_ROWS * ROW_F4 + EMAX_F4) * 16 <= kLdsLimit, "table and bound table fit LDS");
    __shared__ float4 tab[LDS_ROWS * ROW_F4 + EMAX_F4];

    const float NINF = -__builtin_inff();
    const int lane = threadIdx.x & 63;
    const int gl = lane & (G - 1);
    const bool leader = gl == 0;

    // Stage the emission table (already in kernel layout) into LDS once per workgroup.
    for (int i = threadIdx.x; i < LDS_ROWS * ROW_F4 + EMAX_F4; i += WAVES * 64) tab[i] = a.etab[i];
    __syncthreads();

    const uint8_t* __restrict__ res = a.residues;
    const float trBMk = a.tr_B_Mk, tEC = a.tr_E_C, tEJ = a.tr_E_J;
    const bool sameEJ = __float_as_uint(tEC) == __float_as_uint(tEJ);  // wave-uniform (SGPR)

    uint32_t rows_done = 0;  // rows issued by this wave (diagnostics)
    // Work distribution: a group's first sequence is its group number; the index of its next sequence
    // is fetched while the current one runs.  Long rows (S >= 64) fetch it 8 + 256/S rows before the
    // end -- enough to hide the atomic's round trip, late enough that the last indices go to the
    // groups actually about to finish rather than to every group half-way through its sequence:
    // cfg5 25.50 -> 25.03 ms, cfg3 neutral.  Short rows fetch half-way: their sequences end ~100 per
    // us, and at that rate the one counter's atomics queue for more than 17 rows of 28 states
    // (400.hmm x 100k: 1.034 vs 1.004 ms late; profiles/r02_ab_fetch_ahead.jsonl).
    constexpr uint32_t kFetchAhead = S >= 64 ? 8 + 256 / S : 0xFFFFFFFFu;
    constexpr uint32_t kNone = 0xFFFFFFFFu;
    const uint32_t n_groups = MSV_BLOCKS * (WAVES * 64 / G);  // statically assigned first indices
    // The group's first sequence (the first stream's begin consumes it).  With the longest-first order,
    // neighbouring indices have similar lengths.  Wave w of a block runs on SIMD (w mod 4), so the block's
    // waves are dealt in rounds of 4 (one per SIMD): wave w of block b takes the wave-set (64/G
    // consecutive indices) r * 4 * MSV_BLOCKS + 4 * b + (w mod 4), r = w / 4.  The groups of a wave and
    // the 4 SIMDs of a round get similar lengths; successive rounds (the waves sharing a SIMD) come from
    // different parts of the order.  (Block b taking indices [b * groups, ...) gave the 16 waves of a
    // 64-lane-plan block, 4 per SIMD, the 16 longest sequences of the batch: 1400.hmm x 8192 0.66 vs
    // 0.46 ms, 1901.hmm x 256 0.44 vs 0.26 ms; dealing single groups over blocks put each block's
    // longest sequences on one SIMD: cfg2 0.105 vs 0.185 ms -- profiles/r02_ab_first_assignment.jsonl.)
    // Batches larger than the grid (the counter hands out the rest) keep block b on indices [b * groups,
    // ...): there the first sequences all have about the same length, and the rounds measured 0.4-1%
    // slower on cfg3/cfg5.
    static_assert(WAVES % 4 == 0, "waves are dealt in rounds of one per SIMD");
    const uint32_t wave = threadIdx.x >> 6;
    const uint32_t wave_set = a.n <= n_groups ? (wave >> 2) * 4u * MSV_BLOCKS + 4u * MSV_BLOCK + (wave & 3u)
                                              : MSV_BLOCK * WAVES + wave;
    uint32_t pending = wave_set * (64 / G) + static_cast<uint32_t>(lane / G);

    // Drain tail.  The waves of a block are arbitrated oldest-first on their SIMD, so the youngest
    // quarter issue last: a sequence they take near the end of the queue finishes last and sets the
    // launch's end (cfg3 timeline: waves 12-15 did a fifth of the rows of waves 0-3 and still ended
    // 90 us after them -- profiles/r02_wave_timeline_cfg3.jsonl).  For large profiles (S >= 64, whose
    // rows are long enough that fewer waves still keep the SIMD issuing) those waves stop taking
    // sequences once fewer than n_groups * kYoung / 4 remain and leave them to the older
    // waves: cfg3 2.93 -> 2.88 ms, the other large profiles within 0.3%.  Small profiles stay
    // issue-bound to the end (cfg2 lost 9%), so they keep every wave -- profiles/r02_ab_young_cutoff.jsonl.
    constexpr uint32_t kYoung = S >= 64 ? 8 : 0;
    const bool young = kYoung > 0 && (threadIdx.x >> 6) >= (3u * WAVES) / 4u;
    auto take = [&]() __attribute__((always_inline)) -> uint32_t {
        if constexpr (kYoung > 0) {
            if (young) {
                const uint32_t cur = group_take<G>(a.counter, false, lane, n_groups);  // +0: a read
                if (static_cast<uint64_t>(cur) + (static_cast<uint64_t>(n_groups) * kYoung) / 4 >= a.n)
                    return 0xFFFFFFFEu;  // >= n: retire
            }
        }
        return group_take<G>(a.counter, leader, lane, n_groups);
    };
    using Ph0 = std::integral_constant<int, 0>;
    const uint32_t blk_lane = static_cast<uint32_t>(gl & (BLKN > 0 ? BLKN - 1 : 0));  // BLK: the lane's row in a block
    // WIDE: the lane's dword of a superblock at byte a (relative to the stream's base), clamped so that
    // it never reads past the sequence's last residue `endpos` (e3 = max(endpos, 3) - 3; the host runs
    // the twin only on residue buffers of at least 64 bytes): a lane straddling the end loads the last
    // 4 bytes and shifts its own ones down; lanes wholly past the end (or before the buffer start, whose
    // address wrapped) hold garbage rows that are never read.
    std::conditional_t<WIDE, WideBlocks, NoWideBlocks> wb;  // WIDE only (one stream: D == 1)
    std::conditional_t<LAZY, LazyE, NoLazyE> lz;            // LAZY only (one stream: D == 1)
    // The shift is returned separately (`sh`, bits) so a superblock requested ahead is not waited for
    // where it is requested: it is applied when the superblock becomes current.
    auto load_w = [&](uint32_t a, uint32_t e3, uint32_t& sh) __attribute__((always_inline)) -> uint32_t {
        const uint32_t a2 = min(a, e3);
        uint32_t w;
        __builtin_memcpy(&w, res + a2, 4);
        sh = (a - a2) << 3;
        return w;
    };
    // WIDE: 16-row block k (0..3) of a superblock, this lane's row (16k + blk_lane) as a byte code.
    // (only computed for WIDE: left to CSE, the lane term moved the other variants' register assignment)
    const uint32_t bp_lane = WIDE ? static_cast<uint32_t>(((lane & ~15) + (blk_lane >> 2)) << 2) : 0u;
    const uint32_t bp_shift = WIDE ? (blk_lane & 3u) << 3 : 0u;
    auto extract = [&](uint32_t w, uint32_t k) __attribute__((always_inline)) -> uint32_t {
        const uint32_t v = static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute(static_cast<int>(bp_lane + (k << 4)),
                                                                              static_cast<int>(w)));
        return __builtin_amdgcn_ubfe(v, bp_shift, 8);
    };

    // Start the next non-empty sequence in a stream (or retire the stream); `ph` is the phase of the
    // row that will run next (its residue goes to slot r[ph]).
    auto begin = [&](St& st, auto ph) __attribute__((always_inline)) {
        constexpr int PH = decltype(ph)::value;
        // Loop-free on purpose: a retry loop around the group broadcast here was unswitched by
        // the compiler into per-lane copies (see group_take).  An empty (or too long) record
        // instead becomes a one-row "junk" stream: its score is written now, one row is computed
        // on neutral state and discarded, and the stream then restarts with the next index.
        uint32_t idx = pending;
        pending = kNone;
        if (idx == kNone) idx = take();
        const bool retire = idx >= a.n;
        uint32_t s = 0;
        uint64_t o0 = 0, o1 = 0;
        bool bad = false;  // an order entry outside the batch: reported, never dereferenced
        if (!retire) {
            s = a.order ? a.order[idx] : idx;
            bad = s >= a.n;
            const uint32_t sv = bad ? 0u : s;
            o0 = a.offsets[sv];
            o1 = a.offsets[sv + 1];
        }
        const uint64_t L = o1 - o0;
        const bool empty = !retire && !bad && L == 0;    // C_0 = -inf (MSV_HMM.cpp:86,112)
        const bool too_long = !retire && !bad && L >= a.lentab_n;
        if (leader && bad) {  // NaN in the dequeue slot's score makes the batch's error visible in its scores
            a.scores[idx] = __uint_as_float(0x7fc00000u);
            atomicOr(a.errors, kErrBadOrder);
        }
        if (leader && empty) a.scores[s] = NINF;
        if (leader && too_long) {
            a.scores[s] = __uint_as_float(0x7fc00000u);  // quiet NaN bits
            atomicOr(a.errors, kErrTooLong);
        }
        const bool run = !retire && !bad && !empty && !too_long;
        // A retired or junk stream runs with move = -inf: B = Bt = -inf keeps its rows at -inf, so
        // its J partials never reach N and never force the epilogue's group reduction.
        const float2 lm = run ? a.lentab[L] : make_float2(0.f, NINF);
        st.loop = lm.x;
        st.move = lm.y;
        st.seq = s;
        st.pos = run ? static_cast<uint32_t>(o0) : 0u;
        st.endpos = run ? static_cast<uint32_t>(o1 - 1) : 0u;
        // a junk stream ends after its one row; a retired one never (pos cannot reach 2^32 - 1)
        st.endp = retire ? 0xFFFFFFFFu : (run ? static_cast<uint32_t>(o1) : 1u);
        // the next index is fetched kFetchAhead rows before the end (half-way for shorter sequences;
        // equal to endp when L == 1: begin fetches it)
        st.ev = run ? static_cast<uint32_t>(o1 - min(L >> 1, static_cast<uint64_t>(kFetchAhead))) : st.endp;
#pragma unroll
        for (int k = 0; k < S; ++k) st.M[k] = NINF;
        st.J = NINF;
        st.C = NINF;
        st.N = 0.f;       // dp[0][N] = 0      (MSV_HMM.cpp:96)
        st.B = st.move;   // dp[0][B] = tr_move (MSV_HMM.cpp:97)
        st.active = !retire;
        st.junk = !run;
        if constexpr (LAZY) {  // J = -inf: every row is full until the group has a J
            lz.U = NINF;
            lz.Jg = NINF;
        }
        if constexpr (WIDE) {
            // Block j of the stream = rows base + 16j .. base + 16j + 15, base = pos - PH; superblock m =
            // blocks 4m .. 4m + 3.  cur = block 0, nxt = block 1 (PH = 0: block 0 -- the phase-0 row first
            // moves nxt into cur); the phase-0 step then takes block wr into nxt.
            const uint32_t sb = st.pos - PH + 4u * blk_lane;  // (wraps for lanes before the buffer start)
            wb.e3 = max(st.endpos, 3u) - 3u;
            uint32_t sh;
            wb.wcur = load_w(sb, wb.e3, sh);
            wb.wcur >>= sh;
            wb.wnext = load_w(sb + 64u, wb.e3, wb.nsh);
            wb.snext = sb + 128u;
            st.cur = min(extract(wb.wcur, 0u), static_cast<uint32_t>(kPoisonRow));
            wb.nxw = extract(wb.wcur, PH == 0 ? 0u : 1u);
            wb.wr = PH == 0 ? 1u : 2u;
        } else if constexpr (BLK) {
            // The first row runs at phase PH: cur lane b (b >= PH) = residue pos + b - PH, nxt lane b =
            // pos + 16 + b - PH.  PH = 0: the phase-0 row first moves nxt into cur, so both hold the
            // first block.  (Lanes below PH are never read; max() keeps their index >= pos.)
            const uint32_t ic = max(st.pos + blk_lane, st.pos + PH) - PH;
            const uint32_t in = PH == 0 ? ic : st.pos + blk_lane + (BLKN - PH);
            st.cur = min(static_cast<uint32_t>(res[min(ic, st.endpos)]), static_cast<uint32_t>(kPoisonRow));
            st.nxt = res[min(in, st.endpos)];
        } else {
#pragma unroll
            for (int q = 0; q < St::RPF; ++q) st.r[(PH + q) % St::RPF] = res[min(st.pos + q, st.endpos)];
        }
    };
    // Residue code of the row at phase P (0 <= P < NPH + 2) for a row of phase <= P: BLK reads it from
    // the blocks (clamped to the poison row); otherwise the slot (clamped where the row address is made).
    auto resid = [&](St& st, auto pp) __attribute__((always_inline)) -> uint32_t {
        constexpr int P = decltype(pp)::value;
        if constexpr (BLK) {
            if constexpr (P < BLKN) {
                return row_bcast_lane<P>(st.cur);
            } else {
                if constexpr (WIDE) {
                    return min(row_bcast_lane<P - BLKN>(wb.nxw), static_cast<uint32_t>(kPoisonRow));
                } else {
                    return min(row_bcast_lane<P - BLKN>(static_cast<uint32_t>(st.nxt)), static_cast<uint32_t>(kPoisonRow));
                }
            }
        } else {
            return st.r[P % St::RPF];
        }
    };
    auto init = [&](St& st) {
        st.nbr = NINF;
        begin(st, Ph0{});
    };
    // Row prologue: next residue prefetch, emission row pointer, Bt, the j-1 neighbour, ring fill.
    // LDS row of residue code r for this lane (codes >= 20 -> the poison row).  (A hand-written
    // v_min_sdwa + v_mad_u32_u24 form of this address, and pinning the prefetched residue as a
    // 32-bit value, each measured 2-4% slower on 1400.hmm: they move the residue-load wait.)
    // (SPLIT: the LDS holds rows 0..19 only; codes >= 20 read row 19 there and the +inf poison row
    // of the B table, which still makes the score +inf.)
    // The address is one v_mad_u32_u24 on a hoisted lane byte offset (the index form
    // rr * ROW_F4 + gl compiled to v_mul_u32_u24 + v_or: profiles/r01_ab_row_address.jsonl).
    const uint32_t lds_lane = static_cast<uint32_t>(gl * 16);
    auto lds_row = [&](uint32_t r) -> const float4* {
        // (BLK residues arrive clamped)
        const uint32_t rr = BLK ? r : min(r, static_cast<uint32_t>(SPLIT ? kAminoAcids - 1 : kPoisonRow));
        uint32_t off;
        asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(off) : "v"(rr), "s"(static_cast<uint32_t>(ROW_F4 * 16)), "v"(lds_lane));
        return reinterpret_cast<const float4*>(reinterpret_cast<const char*>(tab) + off);
    };
    // SPLIT: the B table ([21][G][HBP] float2: 2-state halves, so the padding past LENG stays under
    // 2 states per lane; lane-contiguous, read as float4) follows the 20 LDS rows in a.etab; the
    // current row's B halves live in `bring`, requested one row ahead.
    const float2* __restrict__ etabB = reinterpret_cast<const float2*>(a.etab + kAminoAcids * ROW_F4);
    struct BRing {
        float2 v[HB > 0 ? HB : 1];
    } bring;
    const uint32_t b_lane = static_cast<uint32_t>(gl * HBP * 8);  // SPLIT: the lane's B halves, in bytes
    auto fill_b = [&](uint32_t r) {
        if constexpr (SPLIT) {
            // lane-contiguous halves: HBP/2 float4 loads per lane (half the VMEM issues of float2 loads
            // strided by G: cfg5 25.08 vs 25.56 ms, profiles/r01_exp_split_b.jsonl)
            // byte offset = row * (G * HBP * 8) + the lane's hoisted offset: one v_mad_u32_u24
            const uint32_t off = min(r, static_cast<uint32_t>(kPoisonRow)) * static_cast<uint32_t>(G * HBP * 8) + b_lane;
            const float4* bp = reinterpret_cast<const float4*>(reinterpret_cast<const char*>(etabB) + off);
#pragma unroll
            for (int q = 0; q < HBP / 2; ++q) {
                const float4 v = bp[q];
                bring.v[2 * q] = make_float2(v.x, v.y);
                if (2 * q + 1 < HB) bring.v[2 * q + 1] = make_float2(v.z, v.w);
            }
        }
    };
    auto row_ptr = [&](St& st, auto ph) -> const float4* {
        if constexpr (!BIG) {
            return lds_row(resid(st, ph));
        } else {
            const uint32_t rr = min(st.r[0], static_cast<uint32_t>(kPoisonRow));
            return (rr < static_cast<uint32_t>(LDS_ROWS)) ? &tab[rr * ROW_F4 + gl] : &a.etab[rr * ROW_F4 + gl];
        }
    };
    // Request the first chunks of a row (all of it when the ring holds a whole row).
    auto fill_ring = [&](auto& rc, const float4* ep) {
        constexpr int P = std::decay_t<decltype(rc)>::kPF;
#pragma unroll
        for (int q = 0; q < (P < CA ? P : CA); ++q) rc.ring[q] = ep[(CA - 1 - q) * G];
    };
    auto prologue = [&](St& st, auto& rc, const float4* ep, auto ph) {
        (void)ph;
        if constexpr (!BLK) rc.rnext = res[min(st.pos + St::RPF, st.endpos)];
        rc.ep = ep;
        rc.Bt = st.B + trBMk;
        if constexpr (G >= 16) {
            st.nbr = shift_in<G>(st.M[S - 1], st.nbr);
            rc.nbr = st.nbr;
        } else {
            rc.nbr = shift_in<G>(st.M[S - 1], NINF);
        }
        // p0/p1 start from the row's first chunk (a plain max, no -inf seed)
        if constexpr (!XROW) fill_ring(rc, ep);
    };
    // One float4 chunk (states 4c+1 .. 4c+4 of the lane), highest state first so M[k-1] is still
    // the previous row's value; the next chunk is requested PF chunks ahead.
    auto chunk = [&](St& st, auto& rc, auto cc) {
        constexpr int P = std::decay_t<decltype(rc)>::kPF;
        constexpr int c = decltype(cc)::value;
        constexpr int slot = (CA - 1 - c) % P;
        const float4 ev = rc.ring[slot];
        if constexpr (c - P >= 0) rc.ring[slot] = rc.ep[(c - P) * G];
        constexpr int k = 4 * c;
        if constexpr (!BIG && S >= 64) {
            // The chunk's 10 VALU ops in a fixed interleaved order (max, max, add, max, add, max, add,
            // max3, add, max3).  gfx950 issues v_max/v_max3 at half the v_add rate and overlaps the two
            // kinds when they alternate; in isolation the compiler's grouping ([4 max][4 add][2 max3])
            // runs 17.2-18.0 cells/ns/SIMD against 20.0-21.0 for this order (tools/micro/row_sched.hip).
            // Inside the kernel the per-row work and LDS traffic fill most of the grouping's gaps: +1.4%
            // on 1400.hmm (2.924 vs 2.964 ms, interleaved A/B), and slower for small rows and for the
            // G = 64 BIG rows (9.2 vs 7.2 ms), which keep the compiler's schedule.
            // Same IEEE ops as the C++ below: max is exact, so max3(p, a, b) == max(max(p, a), b).
            const float mprev = c == 0 ? rc.nbr : st.M[k > 0 ? k - 1 : 0];
            // first two maxes need no emission: a separate block, so the wait for the chunk's LDS
            // data lands after them
            asm volatile(
                "v_max_f32 %0, %1, %4\n\t"
                "v_max_f32 %1, %2, %4"
                : "+v"(st.M[k + 3]), "+v"(st.M[k + 2]), "+v"(st.M[k + 1])
                : "v"(st.M[k]), "v"(rc.Bt));
            if constexpr (LAZY) {
                // The 8 cell ops alone, in the same max/add interleave: the lane's E maximum is taken over the
                // whole row after its last chunk (epilogue), in one block that a lean row skips with one
                // scalar branch.  (Skipping the two E-partial maxes chunk by chunk cost more than it saved: as
                // a second row body behind one branch the allocator permuted M between the two paths and
                // spilled, 400 B of scratch per lane at S = 88; as scalar branches inside this block, one or two
                // per chunk, cfg3 ran 1.2% / 12% slower than without the skip -- profiles/r08_ab_lazy_e.md.)
                asm volatile(
                    "v_add_f32 %0, %6, %0\n\t"
                    "v_max_f32 %2, %3, %5\n\t"
                    "v_add_f32 %1, %7, %1\n\t"
                    "v_max_f32 %3, %4, %5\n\t"
                    "v_add_f32 %2, %8, %2\n\t"
                    "v_add_f32 %3, %9, %3"
                    : "+v"(st.M[k + 3]), "+v"(st.M[k + 2]), "+v"(st.M[k + 1]), "+v"(st.M[k])
                    : "v"(mprev), "v"(rc.Bt), "v"(ev.w), "v"(ev.z), "v"(ev.y), "v"(ev.x));
            } else if constexpr (!SPLIT && c == CA - 1) {  // the row's first chunk starts the E partials
                asm volatile(
                    "v_add_f32 %0, %8, %0\n\t"
                    "v_max_f32 %2, %3, %7\n\t"
                    "v_add_f32 %1, %9, %1\n\t"
                    "v_max_f32 %3, %6, %7\n\t"
                    "v_add_f32 %2, %10, %2\n\t"
                    "v_max_f32 %4, %0, %1\n\t"
                    "v_add_f32 %3, %11, %3\n\t"
                    "v_max_f32 %5, %2, %3"
                    : "+v"(st.M[k + 3]), "+v"(st.M[k + 2]), "+v"(st.M[k + 1]), "+v"(st.M[k]), "=&v"(rc.p0),
                      "=&v"(rc.p1)
                    : "v"(mprev), "v"(rc.Bt), "v"(ev.w), "v"(ev.z), "v"(ev.y), "v"(ev.x));
            } else {
                asm volatile(
                    "v_add_f32 %0, %8, %0\n\t"
                    "v_max_f32 %2, %3, %7\n\t"
                    "v_add_f32 %1, %9, %1\n\t"
                    "v_max_f32 %3, %6, %7\n\t"
                    "v_add_f32 %2, %10, %2\n\t"
                    "v_max3_f32 %4, %4, %0, %1\n\t"
                    "v_add_f32 %3, %11, %3\n\t"
                    "v_max3_f32 %5, %5, %2, %3"
                    : "+v"(st.M[k + 3]), "+v"(st.M[k + 2]), "+v"(st.M[k + 1]), "+v"(st.M[k]), "+v"(rc.p0),
                      "+v"(rc.p1)
                    : "v"(mprev), "v"(rc.Bt), "v"(ev.w), "v"(ev.z), "v"(ev.y), "v"(ev.x));
            }
            return;
        }
        // small rows and BIG rows: the compiler-scheduled form of the same chunk
        st.M[k + 3] = ev.w + fmaxf(st.M[k + 2], rc.Bt);
        st.M[k + 2] = ev.z + fmaxf(st.M[k + 1], rc.Bt);
        st.M[k + 1] = ev.y + fmaxf(st.M[k], rc.Bt);
        if constexpr (c == 0) {
            st.M[k] = ev.x + fmaxf(rc.nbr, rc.Bt);
        } else {
            st.M[k] = ev.x + fmaxf(st.M[k - 1], rc.Bt);
        }
        if constexpr (!SPLIT && c == CA - 1) {  // the row's first chunk: no -inf seed
            rc.p0 = fmaxf(st.M[k + 3], st.M[k + 2]);
            rc.p1 = fmaxf(st.M[k + 1], st.M[k]);
        } else {
            rc.p0 = fmaxf(fmaxf(rc.p0, st.M[k + 3]), st.M[k + 2]);
            rc.p1 = fmaxf(fmaxf(rc.p1, st.M[k + 1]), st.M[k]);
        }
    };
    // SPLIT: one B half (states SA + 2h + 1, + 2 of the lane), emissions already in registers;
    // processed before the A chunks (higher states first, so M[SA - 1] is still the previous row's),
    // the first one seeds the E partials.
    auto bhalf = [&](St& st, auto& rc, auto hh) {
        constexpr int h = decltype(hh)::value;
        constexpr int k = SA + 2 * h;
        const float2 ev = bring.v[h];
        st.M[k + 1] = ev.y + fmaxf(st.M[k], rc.Bt);
        st.M[k] = ev.x + fmaxf(st.M[k - 1], rc.Bt);
        if constexpr (h == HB - 1) {
            rc.p0 = fmaxf(st.M[k + 1], st.M[k]);
            if constexpr (HB == 1) rc.p1 = NINF;
        } else if constexpr (h == HB - 2) {
            rc.p1 = fmaxf(st.M[k + 1], st.M[k]);
        } else if constexpr ((HB - 1 - h) & 1) {
            rc.p1 = fmaxf(fmaxf(rc.p1, st.M[k + 1]), st.M[k]);
        } else {
            rc.p0 = fmaxf(fmaxf(rc.p0, st.M[k + 1]), st.M[k]);
        }
    };
    // Row epilogue: E over the group, the specials (MSV_HMM.cpp:107-110), cursor advance.
    auto epilogue = [&](St& st, auto& rc, auto ph) {
        if constexpr (LAZY) {
            // (`row` has already put U' into lz.U and the decayed J into lz.Jg.)  A lean row only decays J_l.
            // A full row is the row as it was; the lane's bound then restarts from its exact maximum, and Jg,
            // which stays the group's exact J, is re-read from the lane partials on the rows whose E beats it
            // (a J record: wave-uniformly rare, like J >= N below).
            float Jn = st.J + st.loop;
            if (lz.full != 0) {
                // the lane's maximum over the row it has just written: S / 2 three-way maxes on four chains
                float e4[4] = {st.M[0], st.M[1], st.M[2], st.M[3]};
#pragma unroll
                for (int q = 4; q + 1 < S; q += 2) e4[(q / 2) & 3] = fmaxf(fmaxf(e4[(q / 2) & 3], st.M[q]), st.M[q + 1]);
                const float Elane = fmaxf(fmaxf(e4[0], e4[1]), fmaxf(e4[2], e4[3]));
                const float EJ = Elane + tEJ;
                Jn = fmaxf(Jn, EJ);
                lz.U = Elane;
                if (__builtin_expect(__any(EJ > lz.Jg), 0)) lz.Jg = group_max<G>(Jn);
                if (__builtin_expect(!sameEJ, 0)) {
                    st.C = fmaxf(st.C + st.loop, Elane + tEC);
                    asm volatile("" ::: "memory");  // (as below)
                }
            }
            st.J = Jn;
        } else {
            const float Elane = fmaxf(rc.p0, rc.p1);
            // Per-lane partials (see Stream): J_l, and C_l unless C == J (tr_E_C == tr_E_J, which is
            // always the case for the reference's nu = 2, MSV_HMM.cpp:49-53: then the C and J
            // recurrences are identical and C is read from J at the end).
            const float EJ = Elane + tEJ;
            st.J = fmaxf(st.J + st.loop, EJ);
            if (__builtin_expect(!sameEJ, 0)) {
                st.C = fmaxf(st.C + st.loop, Elane + tEC);
                asm volatile("" ::: "memory");  // keep a real (scalar) branch, not a per-row select
            }
        }
        st.N = st.N + st.loop;
        // B = max(N, J) + move needs the group's J = max_l J_l only if some J_l >= N; otherwise
        // max(N, J) == N exactly.  On random-like sequences J stays below N, so the per-row E/J
        // reduction across lanes (DPP butterfly) leaves the row's dependency chain.
        // (G = 64: a row_bcast:15/31 + v_readlane reduction to an SGPR measured 13% slower on
        // 2405.hmm than the permlane swaps -- the SGPR round trip stalls the row)
        // The common value first and the rare one as an overwrite, so the common path falls through
        // (as an if/else the else-block was laid out of line: two taken branches per row).  The test
        // and branch cost 6% of the cfg2 kernel, 0.5% of cfg3 (profiles/r01_exp_speculative_b.jsonl).
        st.B = st.N + st.move;
        if (__builtin_expect(__any(st.J >= st.N), 0)) st.B = fmaxf(st.N, group_max<G>(st.J)) + st.move;
        ++st.pos;
        if constexpr (BLK) {
            // the blocks advance once per 16 rows (step, phase 0)
        } else if constexpr (ROT) {
            st.r[decltype(ph)::value] = rc.rnext;  // this row's slot now holds the row RPF ahead
        } else {
#pragma unroll
            for (int q = 0; q + 1 < St::RPF; ++q) st.r[q] = st.r[q + 1];
            st.r[St::RPF - 1] = rc.rnext;
        }
    };
    // `ph`: phase of the row that runs next.
    auto finish = [&](St& st, auto ph) __attribute__((always_inline)) {
        // Every lane of the group is here (pos == endp is group-uniform), so the group reduction of
        // the C partials reads only active lanes of the same group.
        // (the copy of J is opaque so the compiler cannot hoist this select into every row)
        float csrc = st.C;
        if (sameEJ) asm volatile("v_mov_b32 %0, %1" : "=v"(csrc) : "v"(st.J));
        const float C = group_max<G>(csrc);
        const float sc = C + st.move;  // dp.back()[C] + tr_move (MSV_HMM.cpp:112)
        if (leader && !st.junk) {
            a.scores[st.seq] = sc;
            if (!(sc <= 3.402823466e38f)) atomicOr(a.errors, kErrBadResidue);  // poison row hit
        }
        begin(st, ph);
    };

    // D independent sequences per lane group ("streams"): their rows interleave chunk by chunk,
    // so one stream's serial per-row section (E butterfly -> J/C/N/B -> Bt) overlaps the other
    // stream's cell updates inside the same wave.
    St s0, s1;
    init(s0);
    if constexpr (D == 2) init(s1);

    uint64_t t_start = 0;
    uint64_t c_start = 0;  // (CLOCK twins only; dead code otherwise)
    if (a.stamps) {
        t_start = __builtin_amdgcn_s_memrealtime();
        if constexpr (CLOCK) c_start = __builtin_amdgcn_s_memtime();
    }

    // (Branch-layout hints -- __builtin_expect on the rare end-of-sequence / prefetch events, or on
    // the LDS-row class for G = 64 -- measured no gain, and 15% LOSS for the latter on 2405.hmm.)

    RowCtx<PF> xr, xr1;  // XROW: the ring persists across rows (XROW2: xr for even phases, xr1 for odd)
    if constexpr (XROW) fill_ring(xr, row_ptr(s0, Ph0{}));
    if constexpr (XROW2) fill_ring(xr1, lds_row(resid(s0, std::integral_constant<int, 1>{})));
    fill_b(s0.r[0]);

    // slot of the residue of the row after a row of phase P
    auto next_slot = [](auto ph) { return (decltype(ph)::value + 1) % St::RPF; };

    // LAZY rows.  In these kernels E has one consumer, the lane's J partial J_l = max(J_l + loop, E_l + tEJ)
    // (C is J: the skip is off unless tr_E_C == tr_E_J), and only max_l J_l is ever read (B when J >= N, the
    // score).  Each lane keeps U >= the maximum of its own states' previous row and Jg = the group's J.
    // Before a row,  U' = emax[r][lane] + max3(U, left, Bt)  bounds the lane's new maximum E_l: every cell is
    // fl(e + max(M_prev, Bt)) with e <= emax, M_prev <= U or = left (the exact M shifted in from the left
    // lane), and fl(x + y) is monotone in both arguments.  The row is LEAN if no lane of the wave has
    // fl(U' + tEJ) > fl(Jg + loop): then fl(E_l + tEJ) <= fl(U' + tEJ) <= fl(Jg + loop) = max_l fl(J_l + loop)
    // for every lane, so dropping the E terms leaves max_l J_l -- hence B, the J >= N test and the score --
    // bit for bit what the full row gives.  A lean row skips the block that takes E_l (S/2 half-rate maxes over
    // the finished row) and the E -> J ops of the epilogue, decays J_l and Jg by loop and keeps U = U'; a full
    // row takes E_l, then U = E_l.  Jg never exceeds the group's J: a lean row's J is fl(J + loop) exactly, and
    // a full row re-reads Jg from the lane partials whenever some E_l + tEJ beats it (epilogue).
    // Never lean: a poison residue (emax = +inf, so the +inf reaches the score and kErrBadResidue); the
    // first rows of a sequence (Jg = -inf).  Retired and junk streams (Bt = -inf: U' = -inf, or NaN under
    // a poison residue) compare as "not greater" and never force a full row.
    const uint64_t lazy_off = sameEJ ? 0ull : ~0ull;  // wave-uniform, loop-invariant: tr_E_C != tr_E_J keeps every row full
    // All chunks of one row, C4-1 .. 0, each step pinned so only the rings' registers are live.
    auto row = [&](St& st, auto& rc, const float4* ep, auto ph) {
        float lazy_em = 0.f;
        if constexpr (LAZY) {
            const uint32_t r = resid(st, ph);
            const uint32_t rr = BLK ? r : min(r, static_cast<uint32_t>(kPoisonRow));  // (BLK residues arrive clamped)
            lazy_em = reinterpret_cast<const float*>(tab + LDS_ROWS * ROW_F4)[rr * G + static_cast<uint32_t>(gl)];
        }
        prologue(st, rc, ep, ph);
        if constexpr (LAZY) {
            lz.U = lazy_em + fmaxf(fmaxf(lz.U, rc.nbr), rc.Bt);
            lz.Jg = lz.Jg + st.loop;
            // (an explicit ordered compare: NaN is "not greater" whatever the floating-point flags)
            lz.full = __builtin_amdgcn_fcmpf(lz.U + tEJ, lz.Jg, 2 /* ogt */) | lazy_off;
        }
        if constexpr (SPLIT) {
            [&]<int... I>(std::integer_sequence<int, I...>) {
                ((bhalf(st, rc, std::integral_constant<int, HB - 1 - I>{}),
                  [&] { if constexpr (I & 1) __builtin_amdgcn_sched_barrier(0); }()),
                 ...);
            }(std::make_integer_sequence<int, HB>{});
            fill_b(st.r[next_slot(ph)]);  // this row's B halves are consumed: request the next row's
            __builtin_amdgcn_sched_barrier(0);
        }
        [&]<int... I>(std::integer_sequence<int, I...>) {
            ((chunk(st, rc, std::integral_constant<int, CA - 1 - I>{}), __builtin_amdgcn_sched_barrier(0)), ...);
        }(std::make_integer_sequence<int, CA>{});
        epilogue(st, rc, ph);
    };

    // Wave-uniform loop condition, refreshed only when a stream finishes.
    bool live = __any(D == 2 ? (s0.active || s1.active) : s0.active);

    // One row of phase P of the single-stream, non-row-class paths (XROW or plain), then its events.
    // Returns whether the wave still has work.
    auto step = [&](auto ph) __attribute__((always_inline)) -> bool {  // always_inline: 16 BLK phases exceed the inliner's budget
        constexpr int PH = decltype(ph)::value;
        constexpr int PN = (PH + 1) % NPH;
        using PhN = std::integral_constant<int, PN>;
        if constexpr (WIDE) {
            if constexpr (PH == 0) {
                // a new 16-row block: the one extracted 16 rows ago becomes current; the next one comes from
                // the current superblock, which rotates every 4 blocks (the superblock after the next one
                // requested then, 64 rows ahead of its first use)
                s0.cur = min(wb.nxw, static_cast<uint32_t>(kPoisonRow));
                const uint32_t k = wb.wr & 3u;
                if (k == 0u) {
                    wb.wcur = wb.wnext >> wb.nsh;
                    wb.wnext = load_w(wb.snext, wb.e3, wb.nsh);
                    wb.snext += 64u;
                }
                wb.nxw = extract(wb.wcur, k);
                ++wb.wr;
            }
        } else if constexpr (BLK && PH == 0) {
            // a new 16-row block: the one loaded 16 rows ago becomes current, the next is requested
            s0.cur = min(static_cast<uint32_t>(s0.nxt), static_cast<uint32_t>(kPoisonRow));
            s0.nxt = res[min(s0.pos + BLKN + blk_lane, s0.endpos)];
        }
        if constexpr (XROW2) {
            RowCtx<PF>& rc = (PH & 1) ? xr1 : xr;
            prologue(s0, rc, nullptr, ph);
            [&]<int... I>(std::integer_sequence<int, I...>) {
                ((chunk(s0, rc, std::integral_constant<int, C4 - 1 - I>{})), ...);
            }(std::make_integer_sequence<int, C4>{});
            // the residue of the row after next (discarded if the sequence ends first)
            fill_ring(rc, lds_row(resid(s0, std::integral_constant<int, PH + 2>{})));
            epilogue(s0, rc, ph);
        } else if constexpr (XROW) {
            prologue(s0, xr, nullptr, ph);
            [&]<int... I>(std::integer_sequence<int, I...>) {
                ((chunk(s0, xr, std::integral_constant<int, C4 - 1 - I>{})), ...);
            }(std::make_integer_sequence<int, C4>{});
            // the residue of the next row (discarded if this row ends the sequence)
            fill_ring(xr, lds_row(resid(s0, std::integral_constant<int, PH + 1>{})));
            epilogue(s0, xr, ph);
        } else {
            RowCtx<PF> c0;
            row(s0, c0, row_ptr(s0, ph), ph);
        }
        // Events: see the generic loop below.  Rows of up to 40 states per lane mark them unlikely, so
        // the rows lie in sequence and the common path falls through (without the hint the layout took
        // two branches per row: 400.hmm x 100k 1.072 -> 1.017 ms, 600.hmm 1.456 -> 1.392, cfg2 -1%;
        // longer rows neutral to 0.8% slower, so they keep the plain test --
        // profiles/r03_ab_unlikely_events.jsonl).
        auto events = [&]() __attribute__((always_inline)) {
            if (s0.pos == s0.ev && s0.ev != s0.endp) {
                if (pending == kNone) pending = take();
                s0.ev = s0.endp;
            }
            if (s0.pos == s0.endp) {
                finish(s0, PhN{});
                if constexpr (XROW2) {  // the new sequence's first two rows
                    fill_ring((PN & 1) ? xr1 : xr, row_ptr(s0, PhN{}));
                    fill_ring((PN & 1) ? xr : xr1, lds_row(resid(s0, std::integral_constant<int, PN + 1>{})));
                } else if constexpr (XROW) {
                    fill_ring(xr, row_ptr(s0, PhN{}));
                }
                if constexpr (SPLIT) fill_b(s0.r[PN]);
            }
            live = __any(s0.active);
        };
        if constexpr (S <= 40) {
            if (G == 64 || __builtin_expect(__any(s0.pos == s0.ev), 0)) events();
        } else {
            if (G == 64 || __any(s0.pos == s0.ev)) events();
        }
        ++rows_done;
        return live;
    };

    while (live) {
        if constexpr (ROT || BLK) {
            // NPH rows per iteration (residue slots, or the 16 rows of a BLK block); stops after any row that retires the wave
            [&]<int... I>(std::integer_sequence<int, I...>) {
                (void)(step(std::integral_constant<int, I>{}) && ...);
            }(std::make_integer_sequence<int, NPH>{});
        } else {
            if constexpr (BIG && G == 64) {
                // One sequence per wave: the residue, hence the table row's home, is wave-uniform, so
                // the LDS rows and the L2 rows run as two separate (scalar-branched) row bodies with
                // precise waits -- no generic loads, no per-lane selects.  An L2 row requests up to 10
                // chunks up front to pay the L2 latency about once per row.
                // (a vector compare with exec masking instead of readfirstlane measured 1.5% slower;
                // reading the class one row early into an SGPR changed nothing; a timing-only form
                // with no class branch at all, wrong scores, ran the row 10% faster)
                const uint32_t rr =
                    __builtin_amdgcn_readfirstlane(min(s0.r[0], static_cast<uint32_t>(kPoisonRow)));
                if (rr < static_cast<uint32_t>(LDS_ROWS)) {
                    RowCtx<PF> c0;
                    row(s0, c0, &tab[rr * ROW_F4 + gl], Ph0{});
                } else {
                    RowCtx<(C4 < 10 ? C4 : 10)> c0;
                    row(s0, c0, &a.etab[rr * ROW_F4 + gl], Ph0{});
                }
            } else if constexpr (D == 1) {
                RowCtx<PF> c0;
                row(s0, c0, row_ptr(s0, Ph0{}), Ph0{});
            } else {
                RowCtx<PF> c0, c1;
                prologue(s0, c0, row_ptr(s0, Ph0{}), Ph0{});
                prologue(s1, c1, row_ptr(s1, Ph0{}), Ph0{});
                [&]<int... I>(std::integer_sequence<int, I...>) {
                    ((chunk(s0, c0, std::integral_constant<int, C4 - 1 - I>{}),
                      chunk(s1, c1, std::integral_constant<int, C4 - 1 - I>{}), __builtin_amdgcn_sched_barrier(0)),
                     ...);
                }(std::make_integer_sequence<int, C4>{});
                epilogue(s0, c0, Ph0{});
                epilogue(s1, c1, Ph0{});
            }
            // Events (one compare per stream and row; the handling is rare and wave-uniformly
            // skipped): the half-way fetch of the next index, then the end of the sequence.  (G = 64:
            // the cursor is wave-uniform and the compares are scalar; there the guard made the
            // compiler copy the whole DP row at the loop latch, +12% per row on 2405.hmm, so it is
            // left out.)
            if (G == 64 || __any(D == 2 ? (s0.pos == s0.ev || s1.pos == s1.ev) : s0.pos == s0.ev)) {
                if (s0.pos == s0.ev && s0.ev != s0.endp) {
                    if (pending == kNone) pending = take();
                    s0.ev = s0.endp;
                }
                if constexpr (D == 2) {
                    if (s1.pos == s1.ev && s1.ev != s1.endp) {
                        if (pending == kNone) pending = take();
                        s1.ev = s1.endp;
                    }
                }
                if (s0.pos == s0.endp) {
                    finish(s0, Ph0{});
                    fill_b(s0.r[0]);
                }
                if constexpr (D == 2) {
                    if (s1.pos == s1.endp) finish(s1, Ph0{});
                }
                live = __any(D == 2 ? (s0.active || s1.active) : s0.active);
            }
            ++rows_done;
        }
    }
    // Self-resetting dequeue counter: the last wave of the grid to leave puts counter[0] (next
    // index) and counter[1] (waves left) back to 0, so the next launch needs no memset.  Every
    // wave's last dequeue atomic has returned before its exit increment.
    if (lane == 0) {
        const uint32_t total = MSV_BLOCKS * WAVES;
        if (atomicAdd(a.counter + 1, 1u) == total - 1) {
            atomicExch(a.counter, 0u);
            atomicExch(a.counter + 1, 0u);
        }
    }
    // Diagnostic only (a.stamps == nullptr in production): per-wave start/end realtime (100 MHz),
    // rows issued, XCC id.  Never read by the kernel; used by tools/wave_timeline.py.
    if (a.stamps && lane == 0) {
        const uint64_t t_end = __builtin_amdgcn_s_memrealtime();
        const uint32_t w = MSV_BLOCK * WAVES + (threadIdx.x >> 6);
        uint32_t xcc = 0, hwid = 0;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
        a.stamps[SW * w + 0] = t_start;
        a.stamps[SW * w + 1] = t_end;
        a.stamps[SW * w + 2] = (static_cast<uint64_t>(hwid) << 32) | rows_done;
        a.stamps[SW * w + 3] = (static_cast<uint64_t>(xcc) << 32) | MSV_BLOCK;
        if constexpr (CLOCK) {  // the CLOCK twin (RPFO = kClockTwin): shader-clock ticks over the wave's life
            a.stamps[SW * w + 4] = c_start;
            a.stamps[SW * w + 5] = __builtin_amdgcn_s_memtime();
        }
    }
