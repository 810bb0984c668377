// p7_forward_row.inc -- the float32 Forward row (p7_rows.h states the recurrence), included as text as the body of
// the row loop `for (uint64_t i = 0; i < L; ++i)` of fwd_kernel, dom_fwd_kernel and aln_fwd_kernel; each kernel's own
// stores follow it.  As a function template the same statements compile to other instruction streams in every variant
// (DESIGN 4.6, work distribution); as text each kernel keeps the stream it had.
//
// From the including scope: p7_kernel_head.inc's names, p7_forward_begin.inc's, the row i, loop and move.  M, I, D,
// the specials N, J, Cc, B and the exponent e2 go from row i to row i + 1 in place.
// Leaves: E, the row's E in the scale of the row's exponent (fwd_kernel ignores it, the recording kernels store it).
const uint32_t ph = static_cast<uint32_t>(i) & 63u;
if (ph == 0 && i != 0) {
    cur = nxt;
    nxt = p7::residue_at(res, L, i + 64 + lane);
}
uint32_t code = __builtin_amdgcn_readlane(cur, ph);
maxcode = code > maxcode ? code : maxcode;
code = code < 19u ? code : 19u;
asm volatile("" : "+v"(rz));
const float Bt = B * a.tBM;
// this lane's first float2 of the residue's match and insert odds
const float2* er;
if constexpr (ELDS) er = etab_s + code * ROW2 + lane;
else er = a.etab + code * ROW2 + lane;
const float2* ir = a.itab + code * ROW2 + lane;

// the previous row's last states, from the lane on the left (k - 1 across the boundary)
const float sM = p7::shift1(M[S - 1]), sI = p7::shift1(I[S - 1]), sD = p7::shift1(D[S - 1]);
// M/I pass, highest slot first, in place: I(k) reads M'(k), I'(k); M(k) reads M'(k-1), I'(k-1),
// D'(k-1).  The B term is added last.
float Es = 0.0f;
#pragma unroll
for (int c = C2 - 1; c >= 0; --c) {
    const float2 tmm = tlds(fwdk::MM_IN, c), tim = tlds(fwdk::IM_IN, c), tdm = tlds(fwdk::DM_IN, c);
    const float2 tmi = tlds(fwdk::MI, c), tii = tlds(fwdk::II, c);
    const float2 e = er[c * kLanes];
    float2 ins = {1.0f, 1.0f};
    if constexpr (ISC) ins = ir[c * kLanes];
#pragma unroll
    for (int h = 1; h >= 0; --h) {
        const int q = 2 * c + h;
        float iv = fmaf(I[q], h ? tii.y : tii.x, M[q] * (h ? tmi.y : tmi.x));
        if constexpr (ISC) iv = iv * (h ? ins.y : ins.x);
        const float pm = q ? M[q - 1] : sM, pi = q ? I[q - 1] : sI, pd = q ? D[q - 1] : sD;
        const float acc = fmaf(pd, h ? tdm.y : tdm.x, fmaf(pi, h ? tim.y : tim.x, pm * (h ? tmm.y : tmm.x)));
        const float m = (h ? e.y : e.x) * (acc + Bt);
        M[q] = m;
        I[q] = iv;
        Es += m;
    }
    if constexpr (FENCE) __builtin_amdgcn_sched_barrier(0);
}
// D pass, lowest slot first, each lane's chain started from an incoming 0
const float sMn = p7::shift1(M[S - 1]);  // this row's M(k-1) for each lane's first slot
#pragma unroll
for (int c = 0; c < C2; ++c) {
    const float2 tmd = tlds(fwdk::MD_IN, c), tdd = tlds(fwdk::DD_IN, c);
    D[2 * c] = c ? fmaf(D[2 * c - 1], tdd.x, M[2 * c - 1] * tmd.x) : sMn * tmd.x;
    D[2 * c + 1] = fmaf(D[2 * c], tdd.y, M[2 * c] * tmd.y);
    if constexpr (FENCE) __builtin_amdgcn_sched_barrier(0);
}
// the lanes' affine maps D_out = a D_in + b, scanned inclusively over the lanes: after step j,
// b is the lane's last D given an incoming 0 at lane l - 2^(j+1) + 1
float b = D[S - 1];
b = fmaf(A[0], p7::shift1(b), b);
#pragma unroll
for (int j = 1; j < kScanSteps; ++j) b = fmaf(A[j], p7::shift_by(b, lane, 1 << j), b);
const float Din = p7::shift1(b);  // the exact D entering this lane (0 into lane 0)
#pragma unroll
for (int c = 0; c < C2; ++c) {
    const float2 dc = tlds(fwdk::DC, c);
    D[2 * c] = fmaf(Din, dc.x, D[2 * c]);
    D[2 * c + 1] = fmaf(Din, dc.y, D[2 * c + 1]);
    Es += D[2 * c];
    Es += D[2 * c + 1];
    if constexpr (FENCE) __builtin_amdgcn_sched_barrier(0);
}
// specials: E is the same in every lane (wave_sum), so J, C, N, B and the rescaling are uniform
float E = p7::wave_sum(Es);
N = N * loop;
J = fmaf(J, loop, E * a.tEJ);
Cc = fmaf(Cc, loop, E * a.tEC);
B = (N + J) * move;
const uint32_t Eb = __builtin_amdgcn_readfirstlane(__float_as_uint(E));
if (p7::past_2_32(Eb)) {
    const uint32_t x = p7::exponent_of(Eb);
    const float down = p7::pow2_minus(x);
#pragma unroll
    for (int q = 0; q < S; ++q) {
        M[q] *= down;
        I[q] *= down;
        D[q] *= down;
    }
    N *= down;
    J *= down;
    Cc *= down;
    B *= down;
    E *= down;  // (for the kernels that record it)
    e2 += static_cast<int32_t>(x);
}
