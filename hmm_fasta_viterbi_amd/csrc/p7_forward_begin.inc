// p7_forward_begin.inc -- everything a sequence carries through its Forward rows starts here, as text before the row
// loop of p7_forward_row.inc: M, I, D, the specials and the scale's exponent.  From the including scope: S and move.
float M[S], I[S], D[S];
#pragma unroll
for (int q = 0; q < S; ++q) M[q] = I[q] = D[q] = 0.0f;
float N = 1.0f, J = 0.0f, Cc = 0.0f, B = move;
int32_t e2 = 0;  // the values are the true ones times 2^-e2
uint32_t maxcode = 0;
