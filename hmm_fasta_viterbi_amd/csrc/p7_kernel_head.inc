// p7_kernel_head.inc -- the head of a kernel on the Forward or the Backward row (p7_rows.h), included as text at the
// top of the kernel's body: the tables into LDS, the scan multipliers into VGPRs, the slot-array accessor and the
// wave's first item.  From the including scope: the constants S, ELDS, WAVES and the kernel's arguments a (etab,
// ttab, scan and the queue's fields).  A workgroup without an item returns from the kernel here.
static_assert(S >= 2 && S % 2 == 0, "S must be even");
constexpr int C2 = S / 2;
constexpr int ROW2 = C2 * kLanes;  // float2 per table row
// long rows: every chunk its own scheduling region, or the scheduler hoists a whole row of loads and spills
constexpr bool FENCE = S > 12;
__shared__ float2 etab_s[ELDS ? kRows * ROW2 : 1];
__shared__ float2 ttab_s[kArrays * ROW2];
__shared__ uint32_t exited_s;
const int lane = threadIdx.x & 63;
const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
const uint64_t total = seqq::list_total(a);
if (seqq::no_item<WAVES>(total)) {
    if (threadIdx.x == 0) seqq::count_leavers<1, 1>(a.counter);
    return;
}

if constexpr (ELDS)
    for (int i = threadIdx.x; i < kRows * ROW2; i += WAVES * 64) etab_s[i] = a.etab[i];
for (int i = threadIdx.x; i < kArrays * ROW2; i += WAVES * 64) ttab_s[i] = a.ttab[i];
if (threadIdx.x == 0) exited_s = 0;
__syncthreads();

float A[kScanSteps];  // this lane's multiplier of every scan step, in VGPRs for the whole launch
#pragma unroll
for (int j = 0; j < kScanSteps; ++j) A[j] = a.scan[j * kLanes + lane];
// `rz` is an opaque zero renewed every row: without it the compiler hoists the loop-invariant LDS loads of
// the slot arrays out of the row loop into VGPRs and spills them
uint32_t rz = 0;
auto tlds = [&](int j, int c) -> float2 { return ttab_s[rz + (j * C2 + c) * kLanes + lane]; };

const uint32_t nwaves = gridDim.x * WAVES;
uint32_t item = blockIdx.x * WAVES + wave;
