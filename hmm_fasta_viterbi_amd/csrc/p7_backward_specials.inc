// p7_backward_specials.inc -- the first half of the float32 Backward row (p7_rows.h states the recurrence), included
// as text in the row loop of dom_bck_kernel and aln_bck_kernel, after the loads of the row's Forward record: the
// residue, the emission products, their sum, the rescaling and the specials.  The kernel's posteriors of the special
// states follow it, p7_backward_cells.inc follows those.
//
// From the including scope: p7_kernel_head.inc's names, p7_backward_begin.inc's, the row i, loop and move.
// Leaves: bB, bE of row i, and lN, lJ, lC = loop times the bN, bJ, bC of row i + 1; P(k) in M, H(k) in I.
uint32_t code = 0;
if (i < L) {
    const uint32_t ph = static_cast<uint32_t>(i) & 63u;
    if (ph == 63u && i != L - 1) {
        cur = nxt;
        nxt = (i >= 127) ? res[((i >> 6) - 1) * 64 + lane] : 0u;
    }
    code = __builtin_amdgcn_readlane(cur, ph);
    code = code < 19u ? code : 19u;
}
asm volatile("" : "+v"(rz));
// this lane's first float2 of the residue's match and insert odds
const float2* er;
if constexpr (ELDS) er = etab_s + code * ROW2 + lane;
else er = a.etab + code * ROW2 + lane;
const float2* ir = a.itab + code * ROW2 + lane;

// P(k) = m bM'(k) in M's registers, H(k) = ins bI'(k) in I's; the lanes' sums of P
float Ps = 0.0f;
#pragma unroll
for (int c = 0; c < C2; ++c) {
    const float2 e = er[c * kLanes];
    M[2 * c] = e.x * M[2 * c];
    M[2 * c + 1] = e.y * M[2 * c + 1];
    Ps += M[2 * c];
    Ps += M[2 * c + 1];
    if constexpr (ISC) {
        const float2 ins = ir[c * kLanes];
        I[2 * c] = ins.x * I[2 * c];
        I[2 * c + 1] = ins.y * I[2 * c + 1];
    }
    if constexpr (FENCE) __builtin_amdgcn_sched_barrier(0);
}
float sigma = p7::wave_sum(Ps);  // wave-uniform: the rescaling below is a scalar branch
const uint32_t Sb = __builtin_amdgcn_readfirstlane(__float_as_uint(sigma));
if (p7::past_2_32(Sb)) {
    const uint32_t x = p7::exponent_of(Sb);
    const float down = p7::pow2_minus(x);
#pragma unroll
    for (int q = 0; q < S; ++q) {
        M[q] *= down;
        I[q] *= down;
    }
    bJ *= down;
    bC *= down;
    bN *= down;
    sigma *= down;
    e2 += static_cast<int32_t>(x);
}
// specials (row L: bC = move, the rest 0 -- sigma is 0 there, M and I being 0)
const float bB = sigma * a.tBM;
const float lJ = bJ * loop, lC = bC * loop, lN = bN * loop;
const float mB = move * bB;
bJ = lJ + mB;
bN = lN + mB;
bC = i == L ? move : lC;
const float bE = fmaf(bJ, a.tEJ, a.tEC * bC);
