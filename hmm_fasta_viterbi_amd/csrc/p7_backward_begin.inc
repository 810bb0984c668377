// p7_backward_begin.inc -- everything a sequence carries through its Backward rows starts here, as text before the row
// loop `for (uint64_t i = L + 1; i-- > 0;)`: bM, bI of the row below (in M, I), D, the specials, the scale's exponent
// and the last two residue blocks.  From the including scope: S, lane, a.residues, o0 and L.
float M[S], I[S], D[S];
#pragma unroll
for (int q = 0; q < S; ++q) M[q] = I[q] = D[q] = 0.0f;
float bJ = 0.0f, bC = 0.0f, bN = 0.0f;
int32_t e2 = 0;  // the values are the true ones times 2^-e2
const uint8_t* res = a.residues + o0;
// residues in 64-row blocks from the back: `cur` holds the block of row i's residue (index i)
const uint64_t top = (L - 1) >> 6;
uint32_t cur = (top * 64 + lane < L) ? res[top * 64 + lane] : 0u;
uint32_t nxt = top ? res[(top - 1) * 64 + lane] : 0u;
