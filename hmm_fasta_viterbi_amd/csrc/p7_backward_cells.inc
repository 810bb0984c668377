// p7_backward_cells.inc -- the second half of the float32 Backward row, included as text behind the kernel's
// posteriors of the special states (they stand before these passes over the slots: behind them, the compiler sinks the
// last pass below the kernel's branch and keeps its table values live across it -- S = 22 spilled).  The D chain from
// the top, the mirrored scan, the fix-up, then bM and bI of row i over P and H.
//
// From the including scope: p7_kernel_head.inc's names, M, I, D and p7_backward_specials.inc's bE.
// D chain from the top, each lane's started from an incoming 0; g(k) = P(k+1)
const float gTop = p7::shift1_down(M[0]);  // the right neighbour's first slot (0 into lane 63)
#pragma unroll
for (int c = C2 - 1; c >= 0; --c) {
    const float2 tdm = tlds(domk::B_DM, c), tdd = tlds(domk::B_DD, c);
    const float g1 = (c == C2 - 1) ? gTop : M[2 * c + 2];
    const float u1 = fmaf(tdm.y, g1, bE);
    D[2 * c + 1] = (c == C2 - 1) ? u1 : fmaf(tdd.y, D[2 * c + 2], u1);
    // state 1 (lane 0, slot 0) is entered by no exit
    const float x0 = (c == 0 && lane == 0) ? 0.0f : bE;
    D[2 * c] = fmaf(tdd.x, D[2 * c + 1], fmaf(tdm.x, M[2 * c + 1], x0));
    if constexpr (FENCE) __builtin_amdgcn_sched_barrier(0);
}
// the lanes' affine maps D_out = a D_in + b scanned inclusively towards lane 0: after step j,
// b is the lane's first D given an incoming 0 at lane l + 2^(j+1)
float b = D[0];
b = fmaf(A[0], p7::shift1_down(b), b);
#pragma unroll
for (int j = 1; j < kScanSteps; ++j) b = fmaf(A[j], p7::shift_down_by(b, lane, 1 << j), b);
const float Din = p7::shift1_down(b);  // the exact D entering this lane from the right (0 into lane 63)
// fix-up, then bM and bI in place, lowest slot first: slot q reads P(q+1), not yet overwritten
#pragma unroll
for (int c = 0; c < C2; ++c) {
    const float2 sf = tlds(domk::B_SFX, c);
    D[2 * c] = fmaf(Din, sf.x, D[2 * c]);
    D[2 * c + 1] = fmaf(Din, sf.y, D[2 * c + 1]);
    if constexpr (FENCE) __builtin_amdgcn_sched_barrier(0);
}
#pragma unroll
for (int c = 0; c < C2; ++c) {
    const float2 tmm = tlds(domk::B_MM, c), tmi = tlds(domk::B_MI, c), tmd = tlds(domk::B_MD, c);
    const float2 tim = tlds(domk::B_IM, c), tii = tlds(domk::B_II, c);
    const float g0 = M[2 * c + 1];
    const float g1 = (c == C2 - 1) ? gTop : M[2 * c + 2];
    const float d1 = (c == C2 - 1) ? Din : D[2 * c + 2];
    const float h0 = I[2 * c], h1 = I[2 * c + 1];
    M[2 * c] = fmaf(tmd.x, D[2 * c + 1], fmaf(tmi.x, h0, fmaf(tmm.x, g0, bE)));
    I[2 * c] = fmaf(tii.x, h0, tim.x * g0);
    M[2 * c + 1] = fmaf(tmd.y, d1, fmaf(tmi.y, h1, fmaf(tmm.y, g1, bE)));
    I[2 * c + 1] = fmaf(tii.y, h1, tim.y * g1);
    if constexpr (FENCE) __builtin_amdgcn_sched_barrier(0);
}
