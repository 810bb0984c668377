// p7_forward_end.inc -- the Forward score of sequence s from its last row, as text behind the row loop of
// p7_forward_row.inc: C move, times 2^e2; +inf and kErrBadResidue when a residue code was outside the tables.
// From the including scope: a.scores, a.errors, s, lane, move and p7_forward_begin.inc's Cc, e2, maxcode.
const float sc = fmaf(static_cast<float>(e2), 0.69314718055994529f, logf(Cc * move));
if (lane == 0) {
    if (maxcode >= 20u) {
        a.scores[s] = __builtin_inff();
        atomicOr(a.errors, msvk::kErrBadResidue);
    } else {
        a.scores[s] = sc;
    }
}
