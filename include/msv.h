/*
 * msv.h -- C-ABI of the MI355X-native MSV (Multiple Segment Viterbi) scoring engine.
 *
 * This is the drop-in boundary for the reference's single hot path, the class
 * MSV_HMM (algorithms/MSV_HMM.hpp:17-44 of IvanTyulyandin/HMM_FASTA_Viterbi).  Plain C types
 * only: no HIP, no torch, no C++ in the signatures.  Every entry point cites the reference
 * interface it replaces.  All functions return an msv_status; nothing prints and continues
 * (the reference's check_errors prints and continues, MSV_HMM.cpp:198-203).
 *
 * Ownership: the caller owns every buffer it passes; the library owns the device buffers held
 * by an msv_profile.  One msv_profile may be used by one host thread at a time (the reference
 * MSV_HMM is likewise not thread-safe, MSV_HMM.hpp:33-34); separate profiles are independent.
 * From that one thread, a profile's device launches may go to any streams: every launch takes
 * its own dequeue counter (one of 8 slots, reused only after the slot's previous launch), so
 * launches of one profile on different streams may overlap.
 *
 * Residues cross the boundary as codes 0..19 in the reference's alphabetical order
 * A C D E F G H I K L M N P Q R S T V W Y (MSV_HMM.cpp:29-31), without the '#' sentinel that
 * the reference prepends (FASTA_protein_sequences.cpp:19-20), in a CSR layout:
 * sequence s is residues[offsets[s] .. offsets[s+1]).
 */
#ifndef MSV_H_
#define MSV_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum msv_status {
    MSV_OK = 0,
    MSV_ERR_INVALID_ARGUMENT = 1, /* null pointer, bad size, bad offsets                       */
    MSV_ERR_IO = 2,               /* file cannot be opened (reference: "Failed to open", Profile_HMM.cpp:50-53) */
    MSV_ERR_PARSE = 3,            /* malformed .hmm / FASTA                                    */
    MSV_ERR_BAD_RESIDUE = 4,      /* residue code >= 20 (reference: std::out_of_range from amino_acid_num.at, MSV_HMM.cpp:101) */
    MSV_ERR_SEQUENCE_TOO_LONG = 5,/* longer than the device transition table (msv_profile_reserve_length) */
    MSV_ERR_UNSUPPORTED_MODEL = 6,/* model length outside the compiled kernel family          */
    MSV_ERR_NO_DEVICE = 7,        /* no HIP device / bad device ordinal                        */
    MSV_ERR_HIP = 8,              /* a HIP runtime call failed                                 */
    MSV_ERR_OUT_OF_MEMORY = 9,
    MSV_ERR_RCCL = 10,            /* an RCCL call failed (multi-GPU context)                   */
    MSV_ERR_NO_CONVERGENCE = 11   /* an iterative fit did not converge (calibration, msv_cal_fit_gumbel) */
} msv_status;

typedef struct msv_hmm msv_hmm;         /* parsed HMMER3 profile (host)            */
typedef struct msv_fasta msv_fasta;     /* parsed FASTA, residues packed as codes  */
typedef struct msv_profile msv_profile; /* device-resident MSV scoring profile     */

/* ---------------------------------------------------------------------------------------- */
/* General                                                                                   */
/* ---------------------------------------------------------------------------------------- */
const char* msv_status_string(msv_status status);
const char* msv_version(void);
msv_status msv_device_count(int* count);

/* ---------------------------------------------------------------------------------------- */
/* Host: HMMER3 profile parser -- replaces Profile_HMM::Profile_HMM (Profile_HMM.cpp:48-60)  */
/* ---------------------------------------------------------------------------------------- */
msv_status msv_hmm_read(const char* path, msv_hmm** out);
void msv_hmm_destroy(msv_hmm* hmm);
/* LENG + 1: includes the dummy node M0 (Profile_HMM.cpp:66-71) */
size_t msv_hmm_model_length(const msv_hmm* hmm);
const char* msv_hmm_name(const msv_hmm* hmm);
/* {msv_mu, msv_lambda, viterbi_mu, viterbi_lambda, forward_theta, forward_lambda} (Profile_HMM.hpp:33-43) */
void msv_hmm_stats(const msv_hmm* hmm, float out6[6]);
/* probabilities exp(-x) as parsed (Profile_HMM.cpp:35-45): [model_length][20], [model_length][20], [model_length][7] */
const float* msv_hmm_match_emissions(const msv_hmm* hmm);
const float* msv_hmm_insert_emissions(const msv_hmm* hmm);
const float* msv_hmm_transitions(const msv_hmm* hmm);
/* the COMPO line, the model's average match composition: 20 probabilities exp(-x), parsed as every other row */
const float* msv_hmm_compo(const msv_hmm* hmm);
/* the 20 background frequencies every log-odds score of the library is taken against (MSV_HMM.cpp:21-27) */
const float* msv_background_frequencies(void);

/* MSV host precompute -- replaces MSV_HMM::MSV_HMM (MSV_HMM.cpp:35-57).
 * emission_scores: caller buffer of 20 * model_length floats, residue-major,
 * emission_scores[r * model_length + k] = logf(p_k[r] / bg[r]); column 0 = -inf. */
msv_status msv_hmm_msv_scores(const msv_hmm* hmm, float* emission_scores, float* tr_B_Mk, float* tr_E_C,
                              float* tr_E_J);

/* Per-sequence transitions -- replaces MSV_HMM::init_transitions_depend_on_seq (MSV_HMM.cpp:59-64);
 * L excludes the '#' sentinel. */
void msv_sequence_transitions(uint64_t L, float* tr_loop, float* tr_move);

/* ---------------------------------------------------------------------------------------- */
/* Host: FASTA reader -- replaces FASTA_protein_sequences (FASTA_protein_sequences.cpp:9-44) */
/* Same record semantics (lines joined, records with a symbol outside the 20 amino acids     */
/* dropped, empty records kept); residues are packed straight into the CSR code stream.     */
/* A '#' inside a record is kept by the reference parser and only fails at scoring time;    */
/* here it is stored as code 255, which the scorer rejects with MSV_ERR_BAD_RESIDUE.         */
/* ---------------------------------------------------------------------------------------- */
msv_status msv_fasta_read(const char* path, msv_fasta** out);
void msv_fasta_destroy(msv_fasta* fasta);
size_t msv_fasta_count(const msv_fasta* fasta);
size_t msv_fasta_rejected(const msv_fasta* fasta);
const uint8_t* msv_fasta_codes(const msv_fasta* fasta);     /* offsets[count] bytes   */
const uint64_t* msv_fasta_offsets(const msv_fasta* fasta);  /* count + 1 entries      */
const char* msv_fasta_header(const msv_fasta* fasta, size_t i); /* header line without '>' */

/* ---- FASTA ingest on the GPU -----------------------------------------------
 * The same records as msv_fasta_read (bit-identical codes, offsets, header spans, rejected count),
 * parsed by a chain of tile-scan kernels from FASTA text resident in HBM, so a batch can go from
 * file bytes to scores without a host-side parse.  Results stay in device memory:
 *   codes   : residues() bytes, offsets: count() + 1 uint64 (the scorer's CSR input as is),
 *   spans   : 2 * count() uint64, (start, length) of each header inside the text (no '>').
 * msv_fasta_parse_device takes text already in device memory (n < 2^32 - 2^16 bytes);
 * msv_fasta_read_device reads a file through pinned 64 MiB pieces (read/copy overlapped) and keeps
 * its own device copy of the text (msv_fasta_device_text).  Synchronous w.r.t. `stream`. */
typedef struct msv_fasta_device msv_fasta_device;
msv_status msv_fasta_parse_device(int device, const uint8_t* d_text, uint64_t n, void* stream,
                                  msv_fasta_device** out);
msv_status msv_fasta_read_device(int device, const char* path, void* stream, msv_fasta_device** out);
void msv_fasta_device_destroy(msv_fasta_device* fasta);
uint64_t msv_fasta_device_count(const msv_fasta_device* fasta);
int msv_fasta_device_device(const msv_fasta_device* fasta);           /* the GPU holding it, -1 for NULL */
uint64_t msv_fasta_device_rejected(const msv_fasta_device* fasta);
uint64_t msv_fasta_device_residues(const msv_fasta_device* fasta);
uint64_t msv_fasta_device_max_length(const msv_fasta_device* fasta);  /* longest record */
const uint8_t* msv_fasta_device_codes(const msv_fasta_device* fasta);          /* device pointer */
const uint64_t* msv_fasta_device_offsets(const msv_fasta_device* fasta);       /* device pointer */
const uint64_t* msv_fasta_device_header_spans(const msv_fasta_device* fasta);  /* device pointer */
const uint8_t* msv_fasta_device_text(const msv_fasta_device* fasta);  /* device copy, or NULL */
/* Copies codes / offsets / spans to host buffers sized as above (any may be NULL). */
msv_status msv_fasta_device_download(const msv_fasta_device* fasta, uint8_t* codes, uint64_t* offsets,
                                     uint64_t* spans);

/* Letters -> codes (A..Y -> 0..19).  Any other byte -> MSV_ERR_BAD_RESIDUE. */
msv_status msv_encode_residues(const char* letters, size_t n, uint8_t* codes_out);

/* ---------------------------------------------------------------------------------------- */
/* Device: the hot path -- replaces MSV_HMM::parallel_run_on_sequence (MSV_HMM.cpp:269-430) */
/* and its 6 OpenCL kernels (MSV_kernels.cl:1-65, MSV_spec_kernels.cl:1-50) with ONE fused   */
/* HIP kernel launch per batch.                                                              */
/* ---------------------------------------------------------------------------------------- */

/* Builds a device-resident profile from the precomputed MSV table (exactly what
 * msv_hmm_msv_scores returns).  model_length = LENG + 1. */
msv_status msv_profile_create(int device, const float* emission_scores, uint32_t model_length, float tr_B_Mk,
                              float tr_E_C, float tr_E_J, msv_profile** out);
/* Convenience: parse-side object straight to a device profile (MSV_HMM(const Profile_HMM&), MSV_HMM.hpp:19). */
msv_status msv_profile_create_from_hmm(int device, const msv_hmm* hmm, msv_profile** out);
void msv_profile_destroy(msv_profile* profile);

typedef struct msv_kernel_info {
    uint32_t model_length;     /* LENG + 1                                           */
    uint32_t lanes_per_group;  /* G: lanes that own one sequence's DP row            */
    uint32_t states_per_lane;  /* S: match states held in registers by each lane     */
    uint32_t waves_per_block;  /* 64-lane waves per workgroup                        */
    uint32_t lds_rows;         /* residue rows of the emission table staged in LDS   */
    uint32_t lds_bytes;        /* LDS used per workgroup                             */
    uint32_t blocks;           /* workgroups per launch (persistent grid)            */
    uint32_t max_length;       /* longest sequence the transition table covers        */
    int device;
    char variant[64];          /* throughput plan: batches above latency_max_n and mid_max_n */
    char latency_variant[64];  /* small-batch plan (one sequence per wave), "" if none      */
    uint32_t latency_blocks;   /* its persistent grid                                    */
    uint64_t latency_max_n;    /* batches of up to this many sequences take it            */
    char mid_variant[64];      /* mid-size plan (two sequences per wave), "" if none        */
    uint32_t mid_blocks;       /* its persistent grid                                    */
    uint64_t mid_max_n;        /* batches above latency_max_n, up to this many, take it   */
    char coop_variant[64];     /* cooperative plan (one sequence per workgroup, its row over 4 waves), "" if none */
    uint32_t coop_blocks;      /* its grid (one workgroup per CU)                          */
    uint64_t coop_max_n;       /* batches of up to this many sequences take it (before the latency plan) */
} msv_kernel_info;
msv_status msv_profile_describe(const msv_profile* profile, msv_kernel_info* out);
/* The kernel variant a batch of n sequences runs (msv_score_batch* / grid launches pick the plan by
 * batch size: latency plan, mid plan, throughput plan); "" for a null profile. */
const char* msv_profile_variant_for(const msv_profile* profile, uint64_t n);

/* The compiled kernel family (template instantiations over G, S, waves; names "msv_g<G>_s<S>_w<W>").
 * msv_profile_create picks the cheapest variant with G*S >= LENG; msv_profile_set_variant forces
 * another one (tuning / tests).  Every variant returns identical scores. */
int msv_variant_count(void);
const char* msv_variant_name(int i);
msv_status msv_profile_set_variant(msv_profile* profile, const char* name);

/* Grow the per-sequence transition table so sequences up to max_length residues can be
 * scored (default 131072). Host logf values, so the device never evaluates logf. */
msv_status msv_profile_reserve_length(msv_profile* profile, uint64_t max_length);

/* Page-locked host memory (visible to every GPU).  Residues and scores in such buffers are read and
 * written by the kernels in place (msv_score_batch: no staging copy, ~0.93 of the HBM-resident rate on
 * the BASELINE configs) -- the allocator for FFI callers that cannot reach hipHostMalloc.  Release with
 * msv_host_free.  (Any page-locked memory works the same: hipHostMalloc, hipHostRegister, torch
 * pin_memory.) */
msv_status msv_host_alloc(size_t bytes, void** out);
msv_status msv_host_free(void* ptr);

/* Host buffers in, host scores out; synchronous.  n = number of sequences; offsets has n+1
 * entries, offsets[0] may be non-zero.  scores[s] = MSV log-odds score of sequence s, exactly
 * MSV_HMM::run_on_sequence (MSV_HMM.cpp:74-113); an empty sequence scores -inf.
 * stream may be NULL (the library's own stream).  Batches of >= 4 Mi residues run as a copy/compute
 * pipeline (H2D of later pieces under the kernels of earlier ones); residues in pinned host memory
 * (hipHostMalloc, torch pin_memory) copy at full PCIe rate without runtime staging.  Pinned `scores`
 * are written by the kernels themselves through their device alias (no D2H copy). */
msv_status msv_score_batch(msv_profile* profile, const uint8_t* residues, const uint64_t* offsets, uint64_t n,
                           float* scores, void* stream);

/* Asynchronous host-buffer scoring for a STREAM of batches (serving): enqueues the H2D of the
 * inputs on the profile's copy stream and the order, kernel and score D2H on one of its two compute
 * streams (consecutive calls alternate, so a call's kernel fills the previous one's drain tail), and
 * returns at once with a ticket; msv_profile_wait(ticket) blocks until that call's scores are in
 * `scores` and returns its kernel-latched errors.  Three staging sets, so the copies of the next calls
 * run back to back under the kernels of the earlier ones; at most 3 calls may be outstanding (a fourth
 * returns MSV_ERR_INVALID_ARGUMENT until the oldest is waited for).  The caller keeps residues/offsets
 * unchanged and does not read scores until the wait; pinned (page-locked) host buffers make the
 * copies truly asynchronous, and pinned `scores` are written by the kernel directly (no D2H; that
 * call's errors are then read from its scores: +inf = bad residue, NaN = too long).  One launch per
 * call: residues < 2^32 - 2^20 bytes. */
msv_status msv_score_batch_async(msv_profile* profile, const uint8_t* residues, const uint64_t* offsets, uint64_t n,
                                 float* scores, uint64_t* ticket);
msv_status msv_profile_wait(msv_profile* profile, uint64_t ticket);

/* Device-resident inputs and output (e.g. hipMalloc'd or torch tensors' data pointers), enqueued
 * on `stream` (a hipStream_t, NULL = the library's stream) without a host synchronisation.
 * residues_len = bytes addressable at d_residues (must be < 2^32 per call; split larger batches).
 * d_order: optional permutation (n uint32) giving the order sequences are dequeued in
 * (e.g. longest first); NULL = input order.  Errors found by the kernel (bad residue code,
 * sequence longer than the table) are latched and returned by msv_profile_check. */
msv_status msv_score_batch_device(msv_profile* profile, const uint8_t* d_residues, uint64_t residues_len,
                                  const uint64_t* d_offsets, uint64_t n, const uint32_t* d_order, float* d_scores,
                                  void* stream);

/* Declares `stream` (a hipStream_t) as this profile's working stream until the next bind (NULL
 * unbinds): the caller guarantees it stays alive while bound.  Launches on a bound stream (and on the
 * library's own streams) skip the per-launch event that orders a counter slot's reuse across streams
 * (recorded lazily instead, only if another stream takes the slot): ~4 us less per launch, 3% of a
 * 10k-sequence 100.hmm batch.  Unbound caller streams stay correct, just with that event. */
msv_status msv_profile_bind_stream(msv_profile* profile, void* stream);

/* Synchronises `stream` and returns (then clears) the errors latched by earlier device calls. */
msv_status msv_profile_check(msv_profile* profile, void* stream);

/* Device helper: writes a longest-first dequeue order for a device CSR batch into d_order
 * (n uint32) using a counting sort on the device.  Enqueued on `stream`. */
msv_status msv_order_longest_first(msv_profile* profile, const uint64_t* d_offsets, uint64_t n, uint32_t* d_order,
                                   void* stream);

/* A GPU-parsed FASTA set (msv_fasta_read_device) scored in place: length table reserved for its
 * longest record, longest-first order, one launch, scores copied to the host (count() floats).
 * The set must live on the profile's device (else MSV_ERR_INVALID_ARGUMENT). */
msv_status msv_score_fasta_device(msv_profile* profile, const msv_fasta_device* fasta, float* scores);

/* ---- profiles x sequences grid ---------------------------------------------
 * Replaces the reference's benchmark loop over every profile for one FASTA set
 * (algorithms/benchmark_MSV.cpp:12-24,31-41: one MSV_HMM per .hmm, each scoring every sequence).
 * Every profile keeps its own compile-time kernel variant (the analog of should_specialize,
 * MSV_HMM.cpp:322-337); the launches are forked onto the profiles' own streams so that small
 * batches of different profiles run concurrently, and joined back into `stream`.
 * scores: [n_profiles][n] row-major (profile-major).  All profiles must live on one device; the
 * same profile may appear more than once (its launches then serialise).  Errors latched by the
 * kernels are reported by msv_profile_check on each profile (the host variant does that itself). */
msv_status msv_score_grid(msv_profile* const* profiles, uint32_t n_profiles, const uint8_t* residues,
                          const uint64_t* offsets, uint64_t n, float* scores, void* stream);
msv_status msv_score_grid_device(msv_profile* const* profiles, uint32_t n_profiles, const uint8_t* d_residues,
                                 uint64_t residues_len, const uint64_t* d_offsets, uint64_t n,
                                 const uint32_t* d_order, float* d_scores, void* stream);

/* ---- several devices from one host thread (SURVEY 8(b) msv_score_batch_multi, 8(e)) ----------
 * The reference has no multi-device path.  Sequences are independent, so a batch is cut into
 * contiguous shards with ~equal residue counts (a prefix-sum split that keeps the output order):
 * bounds[k] .. bounds[k+1] is shard k's sequence range (n_shards + 1 entries, bounds[0] = 0,
 * bounds[n_shards] = n).  Host-only; the torch.distributed path (one process per GPU, RCCL
 * gather) uses the same split (hmm_fasta_viterbi_amd/distributed.py). */
msv_status msv_shard_bounds(const uint64_t* offsets, uint64_t n, uint32_t n_shards, uint64_t* bounds);

/* The lazy-E bound table of a kernel variant with G lanes per sequence and S states per lane (host-only,
 * for tests and tools): out[21 * G], out[r * G + l] = the largest of emission_scores[r][l*S + 1 .. l*S + S]
 * (emission_scores: [20][model_length] as msv_hmm_msv_scores returns it; states past model_length - 1 are
 * ignored, a lane with none gets -inf), row 20 = +inf.  The kernels of long whole-row variants skip a row's
 * E maximum where this bound proves that it cannot raise J. */
msv_status msv_lazy_bound_table(const float* emission_scores, uint32_t model_length, int G, int S, float* out);

/* profiles[k]: the same model created on device k (msv_profile_create_from_hmm(k, ...)).  Shard k
 * of the batch is scored on profiles[k]'s device by its own host thread (upload, longest-first
 * order, one launch, download), all shards concurrently; scores land in input order.  The same
 * device may appear more than once (its shards then share the GPU); the same HANDLE may too, and
 * then scores its shards one after another on one thread. */
msv_status msv_score_batch_multi(msv_profile* const* profiles, uint32_t n_profiles, const uint8_t* residues,
                                 const uint64_t* offsets, uint64_t n, float* scores);

/* ---- several devices from one process, scores gathered over RCCL --------------
 * A context over profiles[k] = the same model created on DISTINCT devices (rank k = profiles[k]'s
 * device; one RCCL communicator per device from ncclCommInitAll).  msv_multi_score_batch cuts the
 * batch into residue-balanced contiguous shards (msv_shard_bounds), one host thread per device uploads
 * its shard and enqueues the longest-first order and the kernel on the context's stream for that
 * device, then ONE RCCL group (ncclSend from every rank, ncclRecv into device 0's buffer at the
 * shard's offset -- exact counts, rank 0 included through a self send/recv) gathers the float scores
 * on device 0, and a single D2H returns them in input order.  A device listed twice is
 * MSV_ERR_INVALID_ARGUMENT (one rank per device); RCCL failures are MSV_ERR_RCCL.  The context
 * holds the profiles by pointer: destroy it before them. */
typedef struct msv_multi msv_multi;
msv_status msv_multi_create(msv_profile* const* profiles, uint32_t n_profiles, msv_multi** out);
msv_status msv_multi_score_batch(msv_multi* multi, const uint8_t* residues, const uint64_t* offsets, uint64_t n,
                                 float* scores);
void msv_multi_destroy(msv_multi* multi);

/* ---- MSV filter P-values -----------------------------------------------------
 * The reference parses STATS LOCAL MSV mu/lambda (data_readers/Profile_HMM.cpp:73-94) and never
 * uses them; its README's intent is the HMMER3 filter pipeline.  This is HMMER3's formula for the
 * MSV stage: null1 score nullsc = L log(p1) + log(1 - p1), p1 = L/(L+1) (float, as p7_bg_NullOne);
 * bits = (score - nullsc) / ln 2 (float); P = Gumbel survival(bits; mu, lambda)
 * = 1 - exp(-exp(-lambda (bits - mu))), with the small-tail branch -> exp(-lambda (bits - mu)).
 * There is no reference implementation to pin against ("parity unpinned"); the device and host
 * paths agree with a float64 restatement in tests/.  Empty sequences (score -inf) give P = 1. */
msv_status msv_pvalues(const float* scores, const uint64_t* offsets, uint64_t n, float mu, float lambda,
                       double* pvalues);
msv_status msv_pvalues_device(int device, const float* d_scores, const uint64_t* d_offsets, uint64_t n, float mu,
                              float lambda, double* d_pvalues, void* stream);

/* MSV filter on the device: the P-value of every score (the formula above, written to d_pvalues when it
 * is not NULL) and the indices of the sequences with P <= threshold written to d_selected (n uint32 of
 * room), their number to *d_count (one device uint32).  d_order (NULL or a permutation of 0..n-1, e.g.
 * msv_order_longest_first's) is the order the survivors are listed in, exactly (a stable compaction, two
 * launches): with the longest-first permutation the Viterbi launch dequeues its survivors longest first
 * and its drain tail is its shortest ones.  The survivors list feeds
 * msv_vit_score_batch_device directly (no host round trip).  `stream` must not be NULL
 * (MSV_ERR_INVALID_ARGUMENT): the profiles' calls take NULL as their own non-blocking stream, which the
 * legacy null stream does not order against, so pass the same explicit stream to the calls it chains. */
msv_status msv_filter_select_device(int device, const float* d_scores, const uint64_t* d_offsets,
                                    const uint32_t* d_order, uint64_t n, float mu, float lambda, double threshold,
                                    double* d_pvalues, uint32_t* d_selected, uint32_t* d_count, void* stream);

/* ---- Viterbi stage -----------------------------------------------------------
 * The reference parses everything a Viterbi filter needs -- insert_emissions and the 7 transitions
 * per node (data_readers/Profile_HMM.hpp:28-29, Profile_HMM.cpp:107-120) and STATS LOCAL VITERBI
 * (Profile_HMM.cpp:86-87) -- and never uses it; its README (README.md:2-3) names the Viterbi algorithm
 * as the project's point.  This stage scores HMMER3's generic local Viterbi (p7_GViterbi's recurrence,
 * multihit local mode) over that parse, with the MSV path's own specials (MSV_HMM.cpp:49-64):
 *   M(i,k) = max(M(i-1,k-1)+tMM, I(i-1,k-1)+tIM, D(i-1,k-1)+tDM, B(i-1)+tr_B_Mk) + match[r][k]
 *   I(i,k) = max(M(i-1,k)+tMI, I(i-1,k)+tII) + insert[r][k]        k < LENG (no I at node LENG)
 *   D(i,k) = max(M(i,k-1)+tMD, D(i,k-1)+tDD)
 *   E = max_k M(i,k) (local exits; D(i,LENG) never exceeds it); J, C, N, B and the final C(L) + tr_move
 *   exactly as MSV_HMM::run_on_sequence (MSV_HMM.cpp:100-112, per-length tr_loop / tr_move).
 * Transition t of node k is read from transition_scores[k * 7 + t] (order m->m m->i m->d i->m i->i d->m
 * d->d, as the .hmm file) for nodes 1 .. LENG-1 only: node 0 (B) enters through tr_B_Mk, node LENG has
 * no successor -- so the '*' entries (which the reference parses as probability 1) are never read.
 * There is no reference implementation ("parity unpinned"): the device scores equal the serial
 * restatement in oracle/ bit for bit, and the stage is pinned statistically against every profile's
 * STATS LOCAL VITERBI (tests/). */
typedef struct msv_vit_profile msv_vit_profile;

typedef enum msv_insert_mode {
    MSV_INSERTS_ZERO = 0,    /* HMMER3's convention: insert emissions score 0 (background)          */
    MSV_INSERTS_LOG_ODDS = 1 /* logf(insert_emissions[k][r] / background[r]) of the reference's parse */
} msv_insert_mode;

/* Score tables of the Viterbi stage from a parsed profile (model_length = M = LENG + 1):
 * match_scores [20][M] (== msv_hmm_msv_scores' table), insert_scores [20][M] (0, or the log-odds),
 * transition_scores [M][7] = logf(parsed probability).  Any output pointer may be NULL. */
msv_status msv_hmm_viterbi_scores(const msv_hmm* hmm, int insert_mode, float* match_scores, float* insert_scores,
                                  float* transition_scores, float* tr_B_Mk, float* tr_E_C, float* tr_E_J);

/* The serial CPU Viterbi of one sequence (this library's own restatement, two rolling rows; the
 * reference-shaped Viterbi_HMM::run_on_sequence in msv_hmm.hpp).  codes 0..19; a code >= 20 gives
 * MSV_ERR_BAD_RESIDUE.  insert_scores NULL = zero insert scores. */
msv_status msv_vit_cpu_score(const float* match_scores, const float* insert_scores, const float* transition_scores,
                             uint32_t model_length, float tr_B_Mk, float tr_E_C, float tr_E_J, const uint8_t* codes,
                             uint64_t L, float* score);

/* Device-resident Viterbi profile.  insert_scores NULL = zero insert scores (MSV_INSERTS_ZERO).  Every
 * transition score the recurrence reads (nodes 1 .. LENG-1) must be <= 0, as log-probabilities are
 * (MSV_ERR_INVALID_ARGUMENT otherwise: the kernel relies on it to leave D(LENG) out of E).
 * Threading, as msv_profile: one host thread at a time; from it, device launches may go to any streams
 * (each takes its own dequeue-counter slot, reused only after that slot's previous launch), so
 * launches of one profile on different streams may overlap. */
msv_status msv_vit_profile_create(int device, const float* match_scores, const float* insert_scores,
                                  const float* transition_scores, uint32_t model_length, float tr_B_Mk, float tr_E_C,
                                  float tr_E_J, msv_vit_profile** out);
msv_status msv_vit_profile_create_from_hmm(int device, const msv_hmm* hmm, int insert_mode, msv_vit_profile** out);
void msv_vit_profile_destroy(msv_vit_profile* profile);
msv_status msv_vit_profile_reserve_length(msv_vit_profile* profile, uint64_t max_length);

typedef struct msv_vit_info {
    uint32_t model_length;    /* LENG + 1                                                   */
    uint32_t states_per_lane; /* S: one sequence per 64-lane wave, 64 * S >= LENG             */
    uint32_t transitions_in_registers; /* of the 7 per-slot transition arrays (the rest in LDS) */
    uint32_t match_in_lds;    /* match scores staged in LDS (else read from L2 every row)    */
    uint32_t insert_scores;   /* informative insert scores (read from L2)                    */
    uint32_t waves_per_block;
    uint32_t blocks;          /* persistent grid of a full launch                           */
    uint32_t lds_bytes;
    uint32_t max_length;
    int device;
    char variant[64];
    /* appended fields (append-only: the round-4 prefix above keeps its offsets) */
    uint32_t scratch_bytes;   /* private (scratch) memory per lane of the variant's kernel: spills or
                                 arrays the compiler could not keep in registers (0 for a healthy variant) */
    uint32_t waves_per_sequence; /* 1, or a team of waves sharing one sequence's row (vit_team.hip) */
} msv_vit_info;
msv_status msv_vit_profile_describe(const msv_vit_profile* profile, msv_vit_info* out);
int msv_vit_variant_count(void);
const char* msv_vit_variant_name(int i);
/* Force one compiled variant (tuning / tests); every variant returns identical scores. */
msv_status msv_vit_profile_set_variant(msv_vit_profile* profile, const char* name);

/* Device-resident batch, enqueued on `stream` (NULL = the library's stream).  d_select (optional): the
 * indices of the sequences to score, *d_select_count of them when d_select_count is given (a device
 * uint32, e.g. msv_filter_select_device's d_count), else n of them; NULL = every sequence.  Scores are
 * written at the sequence's index in d_scores (others untouched).  An empty sequence scores -inf; errors
 * (bad residue: +inf score, too long: NaN, a d_select entry >= n: skipped) are latched for
 * msv_vit_profile_check. */
msv_status msv_vit_score_batch_device(msv_vit_profile* profile, const uint8_t* d_residues, uint64_t residues_len,
                                      const uint64_t* d_offsets, uint64_t n, const uint32_t* d_select,
                                      const uint32_t* d_select_count, float* d_scores, void* stream);
/* As msv_profile_bind_stream: `stream` is this profile's working stream until the next bind (NULL
 * unbinds), kept alive by the caller while bound; launches on it skip the per-launch slot event. */
msv_status msv_vit_profile_bind_stream(msv_vit_profile* profile, void* stream);
/* Host buffers in and out, synchronous (every sequence scored); reports only its own errors (errors of
 * earlier device launches stay latched for msv_vit_profile_check). */
msv_status msv_vit_score_batch(msv_vit_profile* profile, const uint8_t* residues, const uint64_t* offsets, uint64_t n,
                               float* scores, void* stream);
msv_status msv_vit_profile_check(msv_vit_profile* profile, void* stream);

/* The filter pipeline on host buffers (HMMER3's MSV -> Viterbi cascade): MSV scores of every sequence
 * (msv_score_batch_device, longest-first), P-values against (msv_mu, msv_lambda), then the Viterbi
 * score of every sequence with P <= F1; msv_scores[n], passed[n] (0/1) and vit_scores[n] (-inf where not
 * passed) are written, *n_passed = the survivors' count.  Everything between upload and download
 * stays on the device.  msv and vit must live on one device. */
msv_status msv_vit_filter_batch(msv_profile* msv, msv_vit_profile* vit, const uint8_t* residues,
                                const uint64_t* offsets, uint64_t n, float msv_mu, float msv_lambda, double F1,
                                float* msv_scores, uint8_t* passed, float* vit_scores, uint64_t* n_passed);

/* ---- Viterbi traces: one optimal state path per sequence ---------------------------
 * The path runs through the model above: N, B, M/I/D of nodes 1..LENG, E, J, C.  It is reported as
 * domains (one pass B -> M .. M -> E each, in sequence order) plus one op byte per core state visited,
 * 'M' (i+1, k+1), 'I' (i+1) or 'D' (k+1) from (i_from, k_from); a domain's first and last op are 'M'.
 * The specials follow: N loops up to the first domain, J between domains, C after the last.
 * Ties (two predecessors giving the same float) are broken in a fixed order, so the CPU and the GPU
 * report the SAME path: M takes M, I, D, B in that order; I takes M before I; D takes M before D; E the
 * smallest k with M(i,k) == E(i); C and J the loop before E; B takes N before J.  The source of a cell is
 * found by comparing its final value with fl(pred + t) of each candidate in that order.
 * A sequence with L = 0 (score -inf), a bad residue (+inf) or too long for the profile (NaN) has no
 * domains. */
typedef struct msv_vit_domain {
    uint32_t seq;                  /* index of the sequence in the batch                            */
    uint32_t i_from, i_to;         /* 1-based residues emitted by the domain's first and last M     */
    uint32_t k_from, k_to;         /* 1-based nodes of the first and last M                         */
    uint32_t ops_len;              /* core states visited, first and last M included                */
    uint64_t ops_begin;            /* index of the domain's first op in the ops bytes               */
} msv_vit_domain;

/* The serial CPU trace of one sequence (the DP of msv_vit_cpu_score with a pointer matrix, walked back):
 * *score has msv_vit_cpu_score's bits.  Two calls size the output: with domains and ops NULL only the
 * counts are written; then domains[*n_domains] (seq = 0, ops_begin from 0) and ops[*n_ops].  Transition
 * scores of nodes 1 .. LENG-1 must be <= 0 (msv_vit_profile_create's rule). */
msv_status msv_vit_cpu_trace(const float* match_scores, const float* insert_scores, const float* transition_scores,
                             uint32_t model_length, float tr_B_Mk, float tr_E_C, float tr_E_J, const uint8_t* codes,
                             uint64_t L, float* score, uint32_t* n_domains, uint64_t* n_ops, msv_vit_domain* domains,
                             uint8_t* ops);

/* The compiled trace plans, by rising capacity (states = LENG covered); a model runs the first that holds
 * it.  Host-only. */
int msv_vit_trace_plan_count(void);
const char* msv_vit_trace_plan_name(int i);
uint32_t msv_vit_trace_plan_capacity(int i);
/* Back-pointer layout of a plan (host-only arithmetic shared by the device layer and the tests): a cell
 * takes 4 bits (M source 2: 0 M, 1 I, 2 D, 3 B; I source 1: 0 M, 1 I; D source 1: 0 M, 1 D), eight cells
 * a uint32, stored [row][word][lane].  Node k (1-based) of plan i lives in *word, *lane at bit *shift;
 * *words and *lanes are the plan's row shape.  Any output may be NULL. */
msv_status msv_vit_trace_plan_cell(int i, uint32_t k, uint32_t* word, uint32_t* lane, uint32_t* shift, uint32_t* words,
                                   uint32_t* lanes);
/* Workspace bytes of one sequence of L residues under plan i: L rows of words x lanes uint32 plus one
 * uint32 record per row (E's argmax k | C from E << 16 | J from E << 17 | B from J << 18). */
uint64_t msv_vit_trace_sequence_bytes(int i, uint64_t L);
/* Cuts sequences of the given workspace sizes, in order, into chunks of at most workspace_bytes: chunk c
 * is [cuts[c], cuts[c+1]), *n_chunks of them (cuts needs n + 1 entries; NULL: count only).  A sequence
 * that alone exceeds the workspace gives MSV_ERR_OUT_OF_MEMORY. */
msv_status msv_vit_trace_chunk_cuts(const uint64_t* bytes, uint64_t n, uint64_t workspace_bytes, uint64_t* cuts,
                                    uint64_t* n_chunks);

/* Traces of the selected sequences of a host batch, computed on the device (vit_trace.hip), synchronous.
 * select NULL = every sequence (n_select ignored); an entry >= n gives MSV_ERR_INVALID_ARGUMENT.  Results
 * are per select entry, in the caller's order (an index may repeat).  workspace_bytes bounds the device
 * memory for back-pointers (0 = the default, 1 GiB): the selected sequences run in chunks that fit it, and
 * a sequence that alone exceeds it gives MSV_ERR_OUT_OF_MEMORY before anything is launched.
 * MSV_ERR_BAD_RESIDUE / MSV_ERR_SEQUENCE_TOO_LONG are reported as msv_vit_score_batch reports them, and
 * *traces is still returned: the offending entries have no domains, the others are traced. */
typedef struct msv_vit_traces msv_vit_traces;
msv_status msv_vit_trace_batch(msv_vit_profile* profile, const uint8_t* residues, const uint64_t* offsets, uint64_t n,
                               const uint32_t* select, uint64_t n_select, uint64_t workspace_bytes,
                               msv_vit_traces** traces);
uint64_t msv_vit_traces_count(const msv_vit_traces* traces);      /* select entries */
uint64_t msv_vit_traces_domains(const msv_vit_traces* traces);    /* domains in all */
uint64_t msv_vit_traces_ops(const msv_vit_traces* traces);        /* op bytes in all */
/* scores[count], domain_offsets[count + 1] (entry q's domains are [q], [q+1]), domains[], ops[]; any may
 * be NULL. */
msv_status msv_vit_traces_copy(const msv_vit_traces* traces, float* scores, uint64_t* domain_offsets,
                               msv_vit_domain* domains, uint8_t* ops);
void msv_vit_traces_free(msv_vit_traces* traces);

typedef struct msv_vit_trace_info {
    char plan[64];
    uint32_t states_per_lane;
    uint32_t lanes_per_sequence;   /* 64 x the waves of the sequence's workgroup                    */
    uint32_t capacity;             /* states                                                        */
    uint32_t scratch_bytes;        /* of the fill kernel (hipFuncGetAttributes)                     */
    uint32_t words_per_lane;       /* uint32 of back-pointers per lane and row                      */
    uint32_t blocks;               /* resident workgroups = sequences in flight of a full launch    */
    uint32_t lds_bytes;
    uint32_t reserved;
    uint64_t default_workspace_bytes;
} msv_vit_trace_info;
/* The trace plan this profile's model runs. */
msv_status msv_vit_trace_describe(msv_vit_profile* profile, msv_vit_trace_info* out);

/* What the call that made `traces` did on the device: its chunks, the back-pointer bytes written, and the
 * summed device times of the fill launches and of the two walk launches (HIP events). */
typedef struct msv_vit_trace_stats {
    uint64_t chunks;
    uint64_t pointer_bytes;
    float fill_ms, walk_ms;
} msv_vit_trace_stats;
msv_status msv_vit_traces_stats(const msv_vit_traces* traces, msv_vit_trace_stats* out);

/* ---- Forward stage: the summed odds of every alignment, and its P-value -------------
 * The score that decides whether a sequence is a hit: the log (nats) of the sum over EVERY state path of
 * the path's odds, where the Viterbi stage takes the best path only.  Tables and specials are the Viterbi
 * stage's (msv_hmm_viterbi_scores, msv_sequence_transitions); the paths are the Viterbi stage's plus ONE
 * addition: D_k -> E is a local exit at no cost for k = 2..LENG, as in HMMER3's p7_GForward (a max never
 * takes these paths, a sum must count them: STATS LOCAL FORWARD was calibrated with them counted).
 * With x = exp(score) for every table entry (-inf and padding give 0), row i, residue r:
 *   M(i,k) = m[r][k] * (M(i-1,k-1) tMM[k-1] + I(i-1,k-1) tIM[k-1] + D(i-1,k-1) tDM[k-1] + B(i-1) tBM)
 *   I(i,k) = ins[r][k] * (M(i-1,k) tMI[k] + I(i-1,k) tII[k])              k = 1..LENG-1
 *   D(i,k) = M(i,k-1) tMD[k-1] + D(i,k-1) tDD[k-1]                        k = 2..LENG
 *   E(i) = sum_k M(i,k) + sum_{k>=2} D(i,k)
 *   N(i) = N(i-1) loop;  J(i) = J(i-1) loop + E(i) tEJ;  C(i) = C(i-1) loop + E(i) tEC;  B(i) = (N(i) + J(i)) move
 *   N(0) = 1, everything else 0 at row 0;  score = log(C(L) move)
 * The CPU function runs this serially in float64 (tables exp((double)float_score)) and is the reference of
 * every test.  The device computes float32 odds rescaled by exact powers of two; for every finite score
 *   |gpu - cpu64| <= 16 (L + LENG) 2^-24 + 4 2^-24 |cpu64|  nats
 * (DESIGN 4.9 derives it).  A sequence's device score is deterministic: it does not depend on the
 * sequence's place in the batch, on the select list, on the stream or on the run.  Unlike the Viterbi
 * stage's, the variants do NOT return identical scores: S changes the order of summation, so two variants
 * may differ within the tolerance.
 * P-value (HMMER3): bits = (score - nullsc) / ln 2 with msv_pvalues' null1 nullsc; P = 1 when bits < tau,
 * else exp(-lambda (bits - tau)); tau, lambda = STATS LOCAL FORWARD (msv_hmm_stats slots 4 and 5).  The
 * null2 / bias corrections are the bias stage's (last block below); Backward, posterior decoding and domain
 * envelopes are the domain stage's (below). */
typedef struct msv_fwd_profile msv_fwd_profile;

/* The serial float64 CPU Forward of one sequence, arguments as msv_vit_cpu_score.  L = 0 scores -inf; a code
 * >= 20 gives MSV_ERR_BAD_RESIDUE.  The batch form scores a CSR batch on a few host threads. */
msv_status msv_fwd_cpu_score(const float* match_scores, const float* insert_scores, const float* transition_scores,
                             uint32_t model_length, float tr_B_Mk, float tr_E_C, float tr_E_J, const uint8_t* codes,
                             uint64_t L, double* score);
msv_status msv_fwd_cpu_score_batch(const float* match_scores, const float* insert_scores,
                                   const float* transition_scores, uint32_t model_length, float tr_B_Mk, float tr_E_C,
                                   float tr_E_J, const uint8_t* codes, const uint64_t* offsets, uint64_t n,
                                   double* scores);
/* Forward P-values on the host (the formula above). */
msv_status msv_fwd_pvalues(const float* scores, const uint64_t* offsets, uint64_t n, float tau, float lambda,
                           double* pvalues);
/* The D-scan constants of a variant of states_per_lane = S states per lane (host-only, what the device layer
 * uploads): per lane l and slot q (state l S + q + 1), slot_dd[l S + q] = the float32 odds of the d->d
 * transition into the slot (0 where none) and slot_prefix[l S + q] = c_q, the product of the lane's slot_dd
 * 0..q; step_products[j * 64 + l] = step j's multiplier of lane l, the product of the whole-lane products
 * c_{S-1} of lanes max(0, l - 2^j + 1) .. l (j = 0..5).  Any output may be NULL. */
msv_status msv_fwd_scan_constants(const float* transition_scores, uint32_t model_length, uint32_t states_per_lane,
                                  float* slot_dd, float* slot_prefix, float* step_products);

/* Device-resident Forward profile; arguments, threading and streams as msv_vit_profile_create.  The compiled
 * variants cover LENG <= 2432 (all bundled profiles); beyond, MSV_ERR_UNSUPPORTED_MODEL. */
msv_status msv_fwd_profile_create(int device, const float* match_scores, const float* insert_scores,
                                  const float* transition_scores, uint32_t model_length, float tr_B_Mk, float tr_E_C,
                                  float tr_E_J, msv_fwd_profile** out);
msv_status msv_fwd_profile_create_from_hmm(int device, const msv_hmm* hmm, int insert_mode, msv_fwd_profile** out);
void msv_fwd_profile_destroy(msv_fwd_profile* profile);
msv_status msv_fwd_profile_reserve_length(msv_fwd_profile* profile, uint64_t max_length);

typedef struct msv_fwd_info {
    uint32_t model_length;    /* LENG + 1                                                   */
    uint32_t states_per_lane; /* S: one sequence per 64-lane wave, 64 * S >= LENG             */
    uint32_t match_in_lds;    /* match odds staged in LDS (else read from L2 every row)      */
    uint32_t insert_scores;   /* informative insert odds (read from L2)                      */
    uint32_t waves_per_block;
    uint32_t blocks;          /* persistent grid of a full launch                           */
    uint32_t lds_bytes;
    uint32_t scratch_bytes;   /* private memory per lane of the variant's kernel (0: no spills) */
    uint32_t max_length;
    int device;
    char variant[64];
} msv_fwd_info;
msv_status msv_fwd_profile_describe(const msv_fwd_profile* profile, msv_fwd_info* out);
int msv_fwd_variant_count(void);
const char* msv_fwd_variant_name(int i);
/* Force one compiled variant (tuning / tests).  Variants may differ within the tolerance above. */
msv_status msv_fwd_profile_set_variant(msv_fwd_profile* profile, const char* name);

/* As msv_vit_score_batch_device: d_select / d_select_count choose the sequences, scores are written at the
 * sequence's index (others untouched).  An empty sequence scores -inf; a bad residue (+inf), a sequence too
 * long for the profile (NaN), a d_select entry >= n (skipped) and a count beyond n (clamped) are latched for
 * msv_fwd_profile_check. */
msv_status msv_fwd_score_batch_device(msv_fwd_profile* profile, const uint8_t* d_residues, uint64_t residues_len,
                                      const uint64_t* d_offsets, uint64_t n, const uint32_t* d_select,
                                      const uint32_t* d_select_count, float* d_scores, void* stream);
msv_status msv_fwd_profile_bind_stream(msv_fwd_profile* profile, void* stream);
/* Host buffers in and out, synchronous (every sequence scored); reports only its own errors. */
msv_status msv_fwd_score_batch(msv_fwd_profile* profile, const uint8_t* residues, const uint64_t* offsets, uint64_t n,
                               float* scores, void* stream);
msv_status msv_fwd_profile_check(msv_fwd_profile* profile, void* stream);
msv_status msv_fwd_pvalues_device(int device, const float* d_scores, const uint64_t* d_offsets, uint64_t n, float tau,
                                  float lambda, double* d_pvalues, void* stream);

/* The full cascade on host buffers: MSV over every sequence; P <= F1 (stats[0..1], STATS LOCAL MSV); Viterbi
 * on those; P <= F2 (stats[2..3], STATS LOCAL VITERBI); Forward on those; Forward P-values (stats[4..5],
 * STATS LOCAL FORWARD) -- `stats` is msv_hmm_stats' six floats.  Written: msv_scores[n], passed_msv[n] (0/1),
 * vit_scores[n] (-inf where not run), passed_vit[n], fwd_scores[n] (-inf where not run), fwd_pvalues[n]
 * (1 where not run) and the two survivor counts.  Everything between the upload and the download stays on
 * the device; the three profiles must live on one device. */
msv_status msv_fwd_filter_batch(msv_profile* msv, msv_vit_profile* vit, msv_fwd_profile* fwd, const uint8_t* residues,
                                const uint64_t* offsets, uint64_t n, const float* stats, double F1, double F2,
                                float* msv_scores, uint8_t* passed_msv, float* vit_scores, uint8_t* passed_vit,
                                float* fwd_scores, double* fwd_pvalues, uint64_t* n_passed_msv,
                                uint64_t* n_passed_vit);

/* ---- Domain stage: Backward, domain posteriors and envelopes of each hit ------------
 * Where a hit's domains are and how many, judged by probability mass over EVERY alignment (the Viterbi
 * trace gives the single best path).  Forward values f are exactly those of the Forward block above.
 * Backward values b are odds: b_X(i) is the summed odds of every completion of a path that is in state X
 * having emitted residues 1..i.  With r = residue i+1, L the length, transitions out of node k for
 * k = 1..LENG-1 (0 elsewhere) and no I at node LENG:
 *   row L:  bC(L) = move;  bE(L) = tEC bC(L);  bJ(L) = bN(L) = bB(L) = 0;  bI(L,k) = 0;  and the silent
 *           chain still runs, k = LENG..1:
 *             bD(L,k) = [k>=2] bE(L) + tDD[k] bD(L,k+1);   bM(L,k) = bE(L) + tMD[k] bD(L,k+1)
 *   row i < L, in this order:
 *           bB(i) = tBM sum_k m[r][k] bM(i+1,k)
 *           bJ(i) = loop bJ(i+1) + move bB(i);  bC(i) = loop bC(i+1);  bN(i) = loop bN(i+1) + move bB(i)
 *           bE(i) = tEJ bJ(i) + tEC bC(i)
 *           i >= 1, k = LENG..1, g(k) = m[r][k+1] bM(i+1,k+1), h(k) = ins[r][k] bI(i+1,k):
 *             bD(i,k) = [k>=2] bE(i) + tDM[k] g(k) + tDD[k] bD(i,k+1)
 *             bM(i,k) = bE(i) + tMM[k] g(k) + tMI[k] h(k) + tMD[k] bD(i,k+1)
 *             bI(i,k) = tIM[k] g(k) + tII[k] h(k)
 * The Backward score is log bN(0); it equals the Forward score up to rounding.  With Z = fC(L) move the
 * per-residue outputs are, for i = 1..L (stored at index i-1 of the sequence's residues):
 *   begin[i] = fB(i-1) bB(i-1) / Z      a domain's first match state emits residue i
 *   end[i]   = fE(i) bE(i) / Z          a domain's last emitted residue is i
 *   occ[i]   = 1 - loop (fN(i-1) bN(i) + fJ(i-1) bJ(i) + fC(i-1) bC(i)) / Z     residue i lies in a domain
 * Envelope rule (HMMER3's posterior heuristic; rt1 = 0.25, rt2 = 0.10 are its defaults): scan j = 1..L
 * with `start` unset and `triggered` false.  While not triggered: if occ[j] - begin[j] < rt2, start = j;
 * else if start is unset, start = j; then, if occ[j] >= rt1, triggered.  While triggered: if
 * occ[j] - end[j] < rt2, the region (start, j) is emitted, start unset, triggered cleared.  A region open
 * at L is not emitted.  Each region carries two serial float sums over its residues in index order:
 * expected_domains = sum begin, mass = sum occ.  Rescoring and aligning an envelope is the alignment stage's
 * (below), its null2 bias correction the bias stage's; splitting a region that holds several domains by stochastic
 * traceback clustering is the split stage's (last block).
 * The CPU function runs all this serially in float64 (odds rescaled by 2^256, as msv_fwd_cpu_score) and is
 * the reference of every test.  The device computes float32 odds rescaled by exact powers of two, Forward
 * and Backward each with its own running exponent; the exponents combine exactly, and for every residue
 *   |gpu - cpu64| <= 48 (L + LENG) 2^-24 + 8 2^-24     absolute, for begin, end and occ
 * (every term is non-negative, each of the three factors f, b, 1/Z carries Forward's relative bound
 * 16 (L + LENG) 2^-24 -- a Backward state step makes no more rounded operations than a Forward one, its
 * scan is as deep -- and every posterior is <= 1; DESIGN 4.10 derives it).  Forward's own bound holds for
 * the Backward score.  The recording Forward kernel returns the Forward kernel's score of the same
 * variant bit for bit.  Device results are deterministic as the Forward stage's are. */
typedef struct msv_dom_profile msv_dom_profile;
typedef struct msv_dom_result msv_dom_result;

typedef struct msv_dom_region {
    uint32_t seq;                  /* index of the sequence in the batch                            */
    uint32_t i_from, i_to;         /* 1-based first and last residue of the region                  */
    float expected_domains;        /* sum of begin over the region                                  */
    float mass;                    /* sum of occ over the region                                    */
} msv_dom_region;

/* The serial float64 CPU decode of one sequence, model arguments as msv_fwd_cpu_score: both scores (nats) and
 * begin / end / occ as double [L]; any output may be NULL.  L = 0 gives -inf scores and writes no per-residue
 * output; a code >= 20 gives MSV_ERR_BAD_RESIDUE.  The batch form decodes a CSR batch on a few host threads;
 * its per-residue outputs are indexed by residue from the batch's first (offsets[s] - offsets[0]). */
msv_status msv_dom_cpu_decode(const float* match_scores, const float* insert_scores, const float* transition_scores,
                              uint32_t model_length, float tr_B_Mk, float tr_E_C, float tr_E_J, const uint8_t* codes,
                              uint64_t L, double* fwd_score, double* bck_score, double* begin, double* end,
                              double* occ);
msv_status msv_dom_cpu_decode_batch(const float* match_scores, const float* insert_scores,
                                    const float* transition_scores, uint32_t model_length, float tr_B_Mk, float tr_E_C,
                                    float tr_E_J, const uint8_t* codes, const uint64_t* offsets, uint64_t n,
                                    double* fwd_scores, double* bck_scores, double* begin, double* end, double* occ);
/* The envelope rule above on the three float arrays of one sequence: THE definition of the rule, which the
 * device kernels reproduce bit for bit on the same arrays.  Two calls size the output as msv_vit_cpu_trace:
 * with regions NULL only *n_regions is written; then regions[*n_regions] (seq = 0). */
msv_status msv_dom_regions(const float* begin, const float* end, const float* occ, uint64_t L, float rt1, float rt2,
                           uint32_t* n_regions, msv_dom_region* regions);
/* The Backward D-scan constants of a variant of states_per_lane = S (host-only, what the device layer uploads;
 * the mirror of msv_fwd_scan_constants): per lane l and slot q (state k = l S + q + 1), slot_dd[l S + q] = the
 * float32 odds of the d->d transition OUT of node k (0 where none), slot_suffix[l S + q] = the product of the
 * lane's slot_dd q..S-1, step_products[j * 64 + l] = the product of the whole-lane products of lanes
 * l .. min(63, l + 2^j - 1) (j = 0..5), computed in float64 from the float32 odds.  Any output may be NULL. */
msv_status msv_dom_scan_constants(const float* transition_scores, uint32_t model_length, uint32_t states_per_lane,
                                  float* slot_dd, float* slot_suffix, float* step_products);
/* Workspace bytes of one selected sequence of L residues: L + 1 rows (row 0 included) of six 32-bit words, the
 * recording kernel's N, J, C, B, E and running exponent.  Chunks are cut by msv_vit_trace_chunk_cuts. */
uint64_t msv_dom_sequence_bytes(uint64_t L);

/* Device-resident domain profile; arguments, threading, streams and variants (S = 2, 6, 12, 22, 38, with and
 * without insert odds, LENG <= 2432) as msv_fwd_profile_create. */
msv_status msv_dom_profile_create(int device, const float* match_scores, const float* insert_scores,
                                  const float* transition_scores, uint32_t model_length, float tr_B_Mk, float tr_E_C,
                                  float tr_E_J, msv_dom_profile** out);
msv_status msv_dom_profile_create_from_hmm(int device, const msv_hmm* hmm, int insert_mode, msv_dom_profile** out);
void msv_dom_profile_destroy(msv_dom_profile* profile);
msv_status msv_dom_profile_reserve_length(msv_dom_profile* profile, uint64_t max_length);

/* Append-only: struct_size is set by the caller to sizeof(msv_dom_info) before the call; the library writes no
 * more than that many bytes, so a caller built against an older header keeps working when fields are added. */
typedef struct msv_dom_info {
    uint32_t struct_size;
    uint32_t model_length;    /* LENG + 1                                                   */
    uint32_t states_per_lane; /* S: one sequence per 64-lane wave, 64 * S >= LENG             */
    uint32_t match_in_lds;    /* match odds staged in LDS (else read from L2 every row)      */
    uint32_t insert_scores;   /* informative insert odds (read from L2)                      */
    uint32_t waves_per_block;
    uint32_t blocks;          /* persistent grid of a full recording launch                 */
    uint32_t backward_blocks; /* persistent grid of a full Backward launch                  */
    uint32_t lds_bytes;       /* of the recording kernel                                    */
    uint32_t backward_lds_bytes;
    uint32_t scratch_bytes;   /* private memory per lane, the larger of the two kernels' (0: no spills) */
    uint32_t max_length;
    int device;
    char variant[64];
} msv_dom_info;
msv_status msv_dom_profile_describe(const msv_dom_profile* profile, msv_dom_info* out);
int msv_dom_variant_count(void);
const char* msv_dom_variant_name(int i);
msv_status msv_dom_profile_set_variant(msv_dom_profile* profile, const char* name);
msv_status msv_dom_profile_bind_stream(msv_dom_profile* profile, void* stream);
msv_status msv_dom_profile_check(msv_dom_profile* profile, void* stream);

/* The recording kernel's Forward score (nothing recorded): arguments and error classes as msv_fwd_score_batch
 * [_device]; the bits are the Forward kernel's of the same S and insert mode. */
msv_status msv_dom_score_batch_device(msv_dom_profile* profile, const uint8_t* d_residues, uint64_t residues_len,
                                      const uint64_t* d_offsets, uint64_t n, const uint32_t* d_select,
                                      const uint32_t* d_select_count, float* d_scores, void* stream);
msv_status msv_dom_score_batch(msv_dom_profile* profile, const uint8_t* residues, const uint64_t* offsets, uint64_t n,
                               float* scores, void* stream);

/* Decode on device buffers, asynchronous on `stream`: two launches (the recording Forward, then Backward) over
 * the sequences of d_select / d_select_count (as msv_fwd_score_batch_device).  Written at the sequence's index:
 * d_fwd_scores, d_bck_scores; at the residue's CSR index (offsets are absolute into these arrays, which hold
 * residues_len floats): d_begin, d_end, d_occ.  d_workspace holds workspace_bytes >= 24 (residues_len + n)
 * bytes (sequence s records its rows from row offsets[s] + s), else MSV_ERR_OUT_OF_MEMORY.  Error classes are
 * Forward's: an empty sequence scores -inf, a bad residue +inf (latched), a too-long sequence NaN (latched), a
 * select entry >= n is skipped (latched); in every error case the sequence's per-residue outputs are untouched. */
msv_status msv_dom_decode_batch_device(msv_dom_profile* profile, const uint8_t* d_residues, uint64_t residues_len,
                                       const uint64_t* d_offsets, uint64_t n, const uint32_t* d_select,
                                       const uint32_t* d_select_count, float* d_fwd_scores, float* d_bck_scores,
                                       float* d_begin, float* d_end, float* d_occ, void* d_workspace,
                                       uint64_t workspace_bytes, void* stream);

/* Decode and envelopes of the selected sequences of a host batch, synchronous.  select NULL = every sequence
 * (n_select ignored); an entry >= n gives MSV_ERR_INVALID_ARGUMENT.  Results are per select entry, in the
 * caller's order (an index may repeat).  workspace_bytes bounds the device memory for the Forward records (0 =
 * the default, 1 GiB): the selected sequences run in chunks that fit it, and a sequence that alone exceeds it
 * gives MSV_ERR_OUT_OF_MEMORY before anything is launched.  The envelope rule runs on the device (one count
 * launch, an exclusive scan, one place launch).  MSV_ERR_BAD_RESIDUE / MSV_ERR_SEQUENCE_TOO_LONG are reported
 * as msv_fwd_score_batch reports them and *result is still returned: the offending entries have their scores'
 * error class, zero posteriors and no regions; the others are decoded. */
msv_status msv_dom_decode_batch(msv_dom_profile* profile, const uint8_t* residues, const uint64_t* offsets, uint64_t n,
                                const uint32_t* select, uint64_t n_select, float rt1, float rt2,
                                uint64_t workspace_bytes, msv_dom_result** result);
uint64_t msv_dom_result_count(const msv_dom_result* result);      /* select entries */
uint64_t msv_dom_result_residues(const msv_dom_result* result);   /* residues of all entries */
uint64_t msv_dom_result_regions(const msv_dom_result* result);    /* regions in all */
/* fwd_scores[count], bck_scores[count], residue_offsets[count + 1] (entry q's posteriors are [q], [q+1]),
 * begin[], end[], occ[] (compacted, entry after entry), region_offsets[count + 1], regions[]; any may be NULL. */
msv_status msv_dom_result_copy(const msv_dom_result* result, float* fwd_scores, float* bck_scores,
                               uint64_t* residue_offsets, float* begin, float* end, float* occ,
                               uint64_t* region_offsets, msv_dom_region* regions);
void msv_dom_result_free(msv_dom_result* result);
/* What the call did on the device: its chunks, the record bytes written, and the summed device times of the
 * recording launches, the Backward launches and the three region launches (HIP events). */
typedef struct msv_dom_stats {
    uint64_t chunks;
    uint64_t record_bytes;
    float forward_ms, backward_ms, regions_ms;
    uint32_t reserved;
} msv_dom_stats;
msv_status msv_dom_result_stats(const msv_dom_result* result, msv_dom_stats* out);

/* ---- Alignment stage: posterior decoding and the optimal-accuracy alignment of an envelope ----
 * What a search reports for a domain: the envelope's own score, its alignment to the model chosen over ALL
 * alignments (not read off the single best path), and how sure each aligned residue is.  This is HMMER3's
 * rescore_isolated_domain: Forward and Backward on the envelope, posterior decoding of every (residue, state)
 * cell, the optimal-accuracy (OA) alignment over those posteriors, and its trace.
 * An ITEM is an envelope: residues i_from .. i_to (1-based, inclusive) of sequence seq, Le = i_to - i_from + 1,
 * decoded as a sequence of its own of Le residues whose loop / move are those of a CONFIGURED length Lc
 * (msv_sequence_transitions(Lc)).  The batch call sets Lc to the parent sequence's length (HMMER never
 * reconfigures the model for an envelope); the CPU functions take Lc.  With Lc = Le an item is a whole sequence
 * and everything below reduces to the Forward and domain blocks above.  With f, b the Forward and Backward odds
 * of those blocks on the Le residues and Z = fC(Le) move:
 *   envelope score = log Z (nats).  HMMER's per-domain score adds (Lc - Le) log(loop), the flanks emitted by N / C.
 *   ppM(i,k) = fM(i,k) bM(i,k) / Z   k = 1..LENG;     ppI(i,k) = fI(i,k) bI(i,k) / Z   k = 1..LENG-1   (D is not decoded)
 *   ppN(i) = fN(i-1) loop bN(i) / Z, likewise ppJ(i), ppC(i): the three terms of 1 - occ(i).  i = 1..Le.
 * Rows are not renormalised: sum_k (ppM + ppI) + ppN + ppJ + ppC = 1 in exact arithmetic.
 * Optimal accuracy, in float32 on float32 posteriors.  A transition is OPEN if its score is finite; "x via t" is
 * x if t is open, else -inf.  Everything is -inf at row 0 except N(0) = 0 and B(0) = 0 via move.  Row i = 1..Le:
 *   M(i,k) = max(M(i-1,k-1) via tMM[k-1], I(i-1,k-1) via tIM[k-1], D(i-1,k-1) via tDM[k-1], B(i-1) via tBM) + ppM(i,k)
 *   I(i,k) = max(M(i-1,k) via tMI[k], I(i-1,k) via tII[k]) + ppI(i,k)
 *   D(i,k) = max(M(i,k-1) via tMD[k-1], D(i,k-1) via tDD[k-1])
 *   E(i) = max_k M(i,k);  N(i) = N(i-1) + ppN(i);  J(i) = max(J(i-1) + ppJ(i), E(i) via tEJ)
 *   C(i) = max(C(i-1) + ppC(i), E(i) via tEC);  B(i) = max(N(i), J(i)) via move
 * The OA score is C(Le), the expected number of correctly labelled residues; accuracy = score / Le.  E takes M
 * only, and that is exact even though Forward counts the D -> E exits: D adds nothing, so a D value on a row is,
 * bit for bit, some M value of the same row to its left, and no D exceeds the row's best M.  It also keeps the
 * trace convention that a domain's first and last op are 'M'.  Each cell is one max and one float add, so the
 * CPU and the GPU agree BIT FOR BIT on the same posterior arrays.  Tie-breaks are the Viterbi trace's: M takes
 * M, I, D, B in that order; I takes M before I; D takes M before D; E the smallest k with M(i,k) == E(i); C and
 * J the loop before E; B takes N before J; the source of a cell is the first candidate in that order that equals
 * the max.  The trace is reported as msv_vit_domain records and op bytes as the Viterbi trace's (an OA path that
 * passes through J yields several domains, all reported), and each op also carries one float32: the posterior of
 * its cell (ppM for 'M', ppI for 'I', 0 for 'D').
 * Tolerances.  The device decodes in float32 odds as the domain stage does and combines a cell as
 * (float) ldexp((double) f (double) b invZ, e_f(i) + e_b(i) - e_f(Le)) with invZ = 1 / (double) Z: the product of
 * two float32 is exact in float64, the exponents combine in an exact ldexp in float64's range (no pair of
 * exponents loses range), and the one float32 rounding of a value <= 1 is at most 2^-24.  For every posterior
 *   |gpu - cpu64| <= 48 (Le + LENG) 2^-24 + 2 2^-24     absolute
 * (each of f, b, 1/Z carries Forward's relative 16 (Le + LENG) 2^-24, every posterior is <= 1; 1 2^-24 for the
 * final rounding, 1 2^-24 covers the float64 roundings and the reference's own).  The OA score against
 * msv_aln_cpu_align: |gpu - cpu| <= Le (posterior bound) + Le^2 2^-24 (a path sums Le posteriors, each within
 * the bound; Le float32 adds of partial sums <= Le).  The envelope score has Forward's bound; with Lc = Le it is
 * the Forward kernel's score of the same variant bit for bit.  Paths are compared exactly, and only against
 * msv_aln_oa on the device's own posteriors.  The null2 bias correction of an envelope is the bias stage's (next
 * block; the `null2` option of msv_aln_align_batch_opts); the stochastic clustering of multi-domain regions is the
 * split stage's (last block). */
typedef struct msv_aln_item {
    uint32_t seq;                  /* index of the parent sequence in the batch                     */
    uint32_t i_from, i_to;         /* 1-based first and last residue of the envelope                */
} msv_aln_item;
typedef struct msv_aln_result msv_aln_result;

/* The serial float64 decode of one envelope (rescaled as msv_dom_cpu_decode), model arguments as
 * msv_fwd_cpu_score: *score = log Z; ppM, ppI double [Le][LENG + 1] (row i - 1, column k; column 0 is 0);
 * ppN, ppJ, ppC double [Le].  Any output may be NULL.  Le = 0 gives -inf and writes nothing else; Lc < Le gives
 * MSV_ERR_INVALID_ARGUMENT, a code >= 20 MSV_ERR_BAD_RESIDUE. */
msv_status msv_aln_cpu_decode(const float* match_scores, const float* insert_scores, const float* transition_scores,
                              uint32_t model_length, float tr_B_Mk, float tr_E_C, float tr_E_J, const uint8_t* codes,
                              uint64_t Le, uint64_t Lc, double* score, double* ppM, double* ppI, double* ppN,
                              double* ppJ, double* ppC);
/* THE definition of the OA alignment and its walk, on float32 posteriors laid out as msv_aln_cpu_decode's (ppM,
 * ppI float [Le][LENG + 1]).  Two calls size the output as msv_vit_cpu_trace: with domains, ops and op_pp NULL
 * only *oa_score and the counts are written; then domains[*n_domains] (seq = 0, i relative to the envelope,
 * ops_begin from 0), ops[*n_ops] and op_pp[*n_ops].  A score that is not finite (no open path to C) has no
 * domains.  The device kernels reproduce this function exactly on the same arrays. */
msv_status msv_aln_oa(const float* ppM, const float* ppI, const float* ppN, const float* ppJ, const float* ppC,
                      const float* transition_scores, uint32_t model_length, float tr_B_Mk, float tr_E_C,
                      float tr_E_J, uint64_t Le, uint64_t Lc, float* oa_score, uint32_t* n_domains, uint64_t* n_ops,
                      msv_vit_domain* domains, uint8_t* ops, float* op_pp);
/* The CPU twin of the whole stage for one item: the float64 decode, rounded to float32 once, then msv_aln_oa. */
msv_status msv_aln_cpu_align(const float* match_scores, const float* insert_scores, const float* transition_scores,
                             uint32_t model_length, float tr_B_Mk, float tr_E_C, float tr_E_J, const uint8_t* codes,
                             uint64_t Le, uint64_t Lc, double* score, float* oa_score, uint32_t* n_domains,
                             uint64_t* n_ops, msv_vit_domain* domains, uint8_t* ops, float* op_pp);
/* Workspace bytes of one item of Le residues under a variant of S = states_per_lane: Le + 1 six-word records,
 * Le rows of 2 S x 64 floats (Forward's fM, fI, then ppM, ppI in place), Le rows of ceil(S / 8) x 64 back-pointer
 * words and Le row records (the Viterbi trace's encoding).  Chunks are cut by msv_vit_trace_chunk_cuts. */
uint64_t msv_aln_item_bytes(uint32_t states_per_lane, uint64_t Le);

/* Aligns envelopes of a host batch on the device (aln_kernel.hip), synchronous: per chunk of items a recording
 * Forward launch (the full fM / fI matrix), a Backward launch that turns it into posteriors in place, an OA fill
 * launch and two walk launches.  The host packs the items' residues into a CSR batch of their own and uploads
 * only those.  Results are per item, in the caller's order; an item may repeat.  seq >= n, i_from < 1,
 * i_to > L or i_from > i_to gives MSV_ERR_INVALID_ARGUMENT before any launch; workspace_bytes bounds the device
 * workspace (0 = 1 GiB) and an item that alone exceeds it gives MSV_ERR_OUT_OF_MEMORY before any launch.
 * MSV_ERR_BAD_RESIDUE is reported as msv_dom_decode_batch reports it and *result is still returned: the
 * offending items have their score's error class and no domains, the others are aligned.  Domains carry the
 * parent's seq and residues relative to the parent.  With keep_posteriors the device's posteriors are kept on
 * the host: 8 Le (LENG + 1) + 12 Le bytes per item. */
msv_status msv_aln_align_batch(msv_dom_profile* profile, const uint8_t* residues, const uint64_t* offsets, uint64_t n,
                               const msv_aln_item* items, uint64_t n_items, uint64_t workspace_bytes,
                               int keep_posteriors, msv_aln_result** result);
uint64_t msv_aln_result_count(const msv_aln_result* result);      /* items */
uint64_t msv_aln_result_domains(const msv_aln_result* result);    /* domains in all */
uint64_t msv_aln_result_ops(const msv_aln_result* result);        /* op bytes in all */
/* envelope_scores[count], oa_scores[count], domain_offsets[count + 1], domains[], ops[], op_pp[]; any may be NULL. */
msv_status msv_aln_result_copy(const msv_aln_result* result, float* envelope_scores, float* oa_scores,
                               uint64_t* domain_offsets, msv_vit_domain* domains, uint8_t* ops, float* op_pp);
/* Item q's posteriors as the device computed them (keep_posteriors, else MSV_ERR_INVALID_ARGUMENT): ppM, ppI
 * float [Le][LENG + 1] as msv_aln_oa takes them, ppN, ppJ, ppC float [Le]; any may be NULL.  An item that was
 * not decoded (its envelope score not finite) has zeros. */
msv_status msv_aln_result_posteriors(const msv_aln_result* result, uint64_t q, float* ppM, float* ppI, float* ppN,
                                     float* ppJ, float* ppC);
void msv_aln_result_free(msv_aln_result* result);

/* Append-only, as msv_dom_info. */
typedef struct msv_aln_info {
    uint32_t struct_size;
    uint32_t states_per_lane;
    uint32_t pointer_words;            /* uint32 of back-pointers per lane and row                 */
    uint32_t forward_blocks, backward_blocks, fill_blocks;   /* persistent grids of full launches */
    uint32_t forward_scratch_bytes, backward_scratch_bytes, fill_scratch_bytes, walk_scratch_bytes;
    uint32_t forward_lds_bytes, backward_lds_bytes, fill_lds_bytes, walk_lds_bytes;
    uint64_t default_workspace_bytes;
    char variant[64];
    uint32_t null2_row_block;          /* R: rows of one unit of aln_null2_partial (bias stage)       */
    uint32_t null2_partial_scratch_bytes, null2_finish_scratch_bytes;
    uint32_t null2_partial_lds_bytes, null2_finish_lds_bytes;
    uint32_t reserved;
} msv_aln_info;
msv_status msv_aln_describe(const msv_dom_profile* profile, msv_aln_info* out);

/* What the call did on the device: its chunks, the matrix bytes the recording launches wrote, and the summed
 * device times of the four launch kinds (HIP events; the walk's two launches together). */
typedef struct msv_aln_stats {
    uint64_t chunks;
    uint64_t matrix_bytes;
    float forward_ms, backward_ms, fill_ms, walk_ms;
} msv_aln_stats;
msv_status msv_aln_result_stats(const msv_aln_result* result, msv_aln_stats* out);

/* ---- Bias stage: the null2 model of an envelope and its corrected scores --------------------------
 * The last step of HMMER3's rescore_isolated_domain: the null2 model of the envelope "by expectation" and the bias
 * correction taken from it, which turns an envelope score into the per-domain bit score and P-value a search
 * reports and, summed over a sequence's domains, into the per-sequence score that decides whether the hit is
 * reported.  It removes the score that composition-biased and low-complexity sequences get from their composition.
 * For an item (envelope) of Le residues and configured length Lc, with the posteriors of the alignment block,
 * m[x][k] / ins[x][k] the FLOAT32 match / insert odds of residue x at node k (insert odds 1 in MSV_INSERTS_ZERO mode):
 *   eM(k) = sum_i ppM(i,k), k = 1..LENG;   eI(k) = sum_i ppI(i,k), k = 1..LENG-1;   eX = sum_i (ppN(i) + ppJ(i) + ppC(i))
 *   null2[x] = (1 / Le) (sum_k eM(k) m[x][k] + sum_k eI(k) ins[x][k] + eX)        x = 0..19  (N, J, C emit at odds 1)
 * which is p7_GNull2_ByExpectation in probability space (the library accepts codes 0..19 only, so the degenerate
 * symbols' averaging has nothing to do).  With n_x the count of x in the envelope:
 *   domcorrection = sum_x n_x log(null2[x])   nats, terms with n_x = 0 skipped
 *   omega = 1/256;   dombias = log(1 + omega exp(domcorrection))
 *   domain bits = (envelope score + (Lc - Le) log loop(Lc) - nullsc(Lc) - dombias) / ln 2, nullsc msv_pvalues' null1;
 *   the domain P-value is Forward's exponential tail on (tau, lambda), exactly as msv_fwd_pvalues computes it.
 *   Per sequence: seqbias = log(1 + omega exp(sum of the domcorrection of its items)),
 *   sequence bits = (Forward score - nullsc - seqbias) / ln 2, with its P-value.
 * A model whose emission scores are all 0 has null2[x] = 1 up to rounding (rows sum to 1), so domcorrection = 0.
 * If every match state gives residue a odds >= c > 1, insert odds are 1 and the envelope is made of a only, then
 * null2[a] >= 1 + (c - 1) sum_k eM(k) / Le > 1: domcorrection > 0 and the corrected bits are below the uncorrected.
 * msv_aln_cpu_null2 runs the float64 decode and the definition in float64 and is the reference of every tolerance.
 * The device (aln_null2.hip) sums the float32 posteriors of the alignment workspace: a unit is (item, block of R =
 * null2_row_block consecutive rows), one wave a unit adds its rows ascending into 2 S + 1 float32 sums per lane and
 * writes a slab; one wave an item adds the slabs in block order, weights, sums across lanes in a fixed butterfly,
 * adds eX and multiplies by 1 / Le.  The float32 order of summation is a function of (S, Le, R) only: a device
 * null2 does not depend on the chunking, the item's place, the grid or the run.  An item whose envelope score is not
 * finite is skipped: its null2 is zeros, its domcorrection 0.
 * Tolerance (DESIGN 4.12 derives it; relative, because every term is non-negative).  With u = 2^-24,
 *   W_x = sum_k m[x][k] + sum_k ins[x][k] + 3   (float64 sums of the float32 odds; ins = 1 for k = 1..LENG-1 without
 *   insert scores) and, for every x,
 *   delta_x = (48 (Le + LENG) + 2 (Le + 2 LENG + 8)) u null2_cpu[x] + W_x 2^-60
 *   |null2_gpu[x] - null2_cpu[x]| <= delta_x
 * (48 (Le + LENG) u: f, b and 1/Z each carry Forward's relative bound; 2 (Le + 2 LENG + 8) u: the float32 sums, the
 * product, the scale and the roundings, for a variant with 2 S <= Le + 4 LENG + 7, which every variant the library
 * picks satisfies; W_x 2^-60: cells that underflow float32 within a row's scale.  That last term is NOT derived: it
 * ASSUMES that the Backward values of one row lie within 2^66 of the row's carrying cell, which the model's
 * transition and emission ranges do not guarantee in general; the final rounding of a posterior alone accounts for
 * W_x 2^-126 of it.  Everything else in the bound follows from the kernels as written.)  And, while delta_x <=
 * null2_cpu[x] / 2 for every residue x that occurs in the item (a condition on the inputs),
 *   |domcorrection_gpu - domcorrection_cpu| <= sum_x n_x delta_x / (null2_cpu[x] - delta_x)
 *                                              + u (|domcorrection_cpu| + that sum) + 2^-149.
 * The device's domcorrection is msv_aln_null2_correction on the device's own null2, bit for bit. */

/* The float64 null2 of one envelope, model arguments as msv_aln_cpu_decode: null2 double [20], *domcorrection in nats;
 * either may be NULL.  Le = 0 or Lc < Le gives MSV_ERR_INVALID_ARGUMENT, a code >= 20 MSV_ERR_BAD_RESIDUE. */
msv_status msv_aln_cpu_null2(const float* match_scores, const float* insert_scores, const float* transition_scores,
                             uint32_t model_length, float tr_B_Mk, float tr_E_C, float tr_E_J, const uint8_t* codes,
                             uint64_t Le, uint64_t Lc, double* null2, double* domcorrection);
/* THE definition of the correction from a float32 null2 vector: counts the residues, sums n_x log((double) null2[x])
 * in float64 for x = 0..19 in that order (n_x = 0 skipped) and rounds once to float32. */
msv_status msv_aln_null2_correction(const float* null2, const uint8_t* codes, uint64_t Le, float* domcorrection);
/* The bias, bit score and P-value arithmetic above, on the host.  Per item q < m: envelope_scores, Le, Lc,
 * domcorrection in; dombias, domain_bits (float), domain_pvalues (double) out.  Per sequence s < n_seq (n_seq may be
 * 0: then nothing per sequence is read or written): parent[q] < n_seq names item q's sequence, fwd_scores and
 * seq_lengths in; seq_bias, seq_bits, seq_pvalues out (a sequence with no item has seqbias log(1 + omega)).  Float
 * where msv_fwd_pvalues is float, the sums of corrections and the logs in float64 rounded once.  Any output may be
 * NULL. */
msv_status msv_aln_bias_scores(const float* envelope_scores, const uint64_t* Le, const uint64_t* Lc,
                               const float* domcorrection, uint64_t m, const uint32_t* parent, const float* fwd_scores,
                               const uint64_t* seq_lengths, uint64_t n_seq, float tau, float lambda, float* dombias,
                               float* domain_bits, double* domain_pvalues, float* seq_bias, float* seq_bits,
                               double* seq_pvalues);

/* Options of msv_aln_align_batch_opts.  Append-only: struct_size is set by the caller to sizeof(msv_aln_options);
 * fields beyond it read as 0.  NULL options are all zeros. */
typedef struct msv_aln_options {
    uint64_t struct_size;
    uint64_t workspace_bytes;  /* as msv_aln_align_batch's (0 = 1 GiB)                                       */
    int32_t keep_posteriors;
    int32_t null2;             /* run the bias stage's two launches per chunk (aln_null2.hip)                */
} msv_aln_options;
/* msv_aln_align_batch with options; msv_aln_align_batch is this call with null2 = 0.  With null2 = 0 no launch or
 * allocation is added and every result byte is msv_aln_align_batch's.  With null2 the slabs of the partial sums live
 * in a device buffer of the call's own, about 1 / null2_row_block of the matrix (never in the workspace: the chunk
 * cuts are unchanged); if it cannot be allocated the call gives MSV_ERR_OUT_OF_MEMORY. */
msv_status msv_aln_align_batch_opts(msv_dom_profile* profile, const uint8_t* residues, const uint64_t* offsets,
                                    uint64_t n, const msv_aln_item* items, uint64_t n_items,
                                    const msv_aln_options* options, msv_aln_result** result);
/* null2 float [count][20] and domcorrection float [count] of a result made with the null2 option (else
 * MSV_ERR_INVALID_ARGUMENT); either may be NULL. */
msv_status msv_aln_result_null2(const msv_aln_result* result, float* null2, float* domcorrection);
/* What the null2 launches did (msv_aln_stats has no size field and stays as it is): append-only as msv_aln_info. */
typedef struct msv_aln_null2_stats {
    uint32_t struct_size;
    uint32_t row_block;        /* R                                                            */
    float null2_ms;            /* summed device time of the two launches of every chunk       */
    float partial_ms;          /* of it, the aln_null2_partial launches'                       */
    uint64_t slab_bytes;       /* the slab buffer the call allocated                           */
} msv_aln_null2_stats;
msv_status msv_aln_result_null2_stats(const msv_aln_result* result, msv_aln_null2_stats* out);

/* ---- Bias filter: HMMER3's composition filter between MSV and Viterbi -----------------------------
 * (Not the "bias stage" above: that is null2, per domain, at the end of the pipeline.  This is its per-sequence
 * counterpart at the front, p7_bg_SetFilter / p7_bg_FilterScore, on by default in hmmsearch.)  A two-state HMM is
 * run by Forward over the sequence: state 0 emits the background, state 1 the profile's average composition (the
 * COMPO line).  Its score replaces null1 in the P-values of the MSV, Viterbi and Forward filters, so that a sequence
 * that passes on composition alone does not reach the expensive stages.  The reference parses for this pipeline
 * and never runs it: the model below is the definition, the float64 CPU twin (msv_bf_cpu_score) the reference of
 * every tolerance, and parity with HMMER is unpinned, as for the Viterbi and Forward stages.
 * For a profile with LENG = M (model_length = M + 1):
 *   compo[x] = exp(-COMPO value), x = 0..19;   f[x] = msv_background_frequencies;   r[x] = compo[x] / f[x] in float64
 *   states 0 (background, emission odds 1) and 1 (biased, emission odds r[x]);  L0 = 400, L1 = M / 8 as floats
 *   t00 = L0/(L0+1)   t01 = 1/(L0+1)   t10 = 1/(L1+1)   t11 = L1/(L1+1)      pi0 = 0.999   pi1 = 0.001
 *   both states go to the end with weight 1 (the length distribution is imposed outside).
 * For residues x_1..x_L, with T = {t00 t01; t10 t11}:
 *   v_1 = (pi0, pi1 r[x_1]);   v_i = (v_{i-1} T) diag(1, r[x_i]);   bias(seq) = log(v_L[0] + v_L[1]) nats;  0 for L = 0.
 * HMMER's filtersc is nullsc + bias, nullsc msv_pvalues' null1, so the filtered bit score of any stage is
 *   bits = (score - nullsc - bias) / ln 2
 * through that stage's own tail: Gumbel (mu, lambda) for MSV and Viterbi, the exponential (tau, lambda) for Forward.
 * A score of -inf gives P = 1 whatever the bias; with bias = 0 every formula is msv_pvalues' / msv_fwd_pvalues', bit
 * for bit.
 * The device (bias_filter.hip): one sequence per wave; the step is a 2x2 matrix product, so a trip of 1,024 residues
 * -- counted from the sequence's first residue, never from its address -- is 64 lane products of 16 steps combined
 * in lane order by a six-level cross-lane butterfly, all in float32, each product normalised by an exact power of
 * two.  A bias is a function of the sequence and the profile alone.  L = 0 writes 0; a code >= 20 writes +inf and
 * latches the bad-residue bit; a select entry >= n is latched and skipped; there is no length limit.
 * Tolerance (DESIGN 4.13 counts the roundings; every term is non-negative, so the bound is relative in the odds and
 * absolute in nats).  With u = 2^-24 and k = 5 L + 14 ceil(L / 1024) + 4, while k u < 1:
 *   |bias_gpu - bias_cpu| <= k u / (1 - k u) + u |bias_cpu|
 * The device needs 2^-24 <= r[x] <= 2^7 for every x (a composition and a background that are distributions give
 * r <= 1 / min f < 88): msv_bf_profile_create gives MSV_ERR_UNSUPPORTED_MODEL otherwise. */
typedef struct msv_bf_profile msv_bf_profile;
enum { MSV_BF_GUMBEL = 0, MSV_BF_EXPONENTIAL = 1 }; /* the tail of a filtered P-value */

/* THE definition, in float64, rescaled by exact powers of two: compo, background 20 floats each (compo finite and
 * >= 0, background finite and > 0, else MSV_ERR_INVALID_ARGUMENT), model_length = LENG + 1 >= 2.  A code >= 20 gives
 * MSV_ERR_BAD_RESIDUE.  The batch form runs it over CSR offsets. */
msv_status msv_bf_cpu_score(const float* compo, const float* background, uint32_t model_length, const uint8_t* codes,
                            uint64_t L, double* bias);
msv_status msv_bf_cpu_score_batch(const float* compo, const float* background, uint32_t model_length,
                                  const uint8_t* codes, const uint64_t* offsets, uint64_t n, double* bias);
/* THE arithmetic of the filtered P-value, in float where msv_pvalues / msv_fwd_pvalues are float: their terms, with
 * "- bias" after "- nullsc".  kind = MSV_BF_GUMBEL (location mu) or MSV_BF_EXPONENTIAL (location tau).  With bias
 * all zero the results are those two calls', bitwise. */
msv_status msv_bf_pvalues(const float* scores, const float* bias, const uint64_t* offsets, uint64_t n, float location,
                          float scale, int kind, double* pvalues);
/* The device table: 26 floats {t00, t01, t10, t11, pi0, pi1, r[0..19]}, each rounded once from float64. */
msv_status msv_bf_device_table(const float* compo, const float* background, uint32_t model_length, float* table);

msv_status msv_bf_profile_create(int device, const float* compo, const float* background, uint32_t model_length,
                                 msv_bf_profile** out);
msv_status msv_bf_profile_create_from_hmm(int device, const msv_hmm* hmm, msv_bf_profile** out);
void msv_bf_profile_destroy(msv_bf_profile* profile);

/* Append-only, as msv_aln_info: struct_size is written by the library. */
typedef struct msv_bf_info {
    uint32_t struct_size;
    uint32_t model_length;
    uint32_t residues_per_lane;  /* c: consecutive residues of a lane per trip */
    uint32_t residues_per_trip;  /* 64 c                                       */
    uint32_t waves_per_block;
    uint32_t blocks;             /* persistent grid of a full launch           */
    uint32_t lds_bytes;
    uint32_t scratch_bytes;
    uint32_t vgprs;
    int device;
    float table[26];             /* msv_bf_device_table                        */
    char variant[64];
} msv_bf_info;
msv_status msv_bf_profile_describe(const msv_bf_profile* profile, msv_bf_info* out);

/* The bias of every sequence of a host batch (one launch), and of a device-resident batch, optionally only the
 * sequences listed at d_select (their count the device word d_select_count, else n), asynchronous on `stream`
 * (NULL: the profile's own): conventions as msv_fwd_score_batch / msv_fwd_score_batch_device.  d_bias is written at
 * the sequence's index; entries of sequences that are not listed are left as they were. */
msv_status msv_bf_score_batch(msv_bf_profile* profile, const uint8_t* residues, const uint64_t* offsets, uint64_t n,
                              float* bias, void* stream);
msv_status msv_bf_score_batch_device(msv_bf_profile* profile, const uint8_t* d_residues, uint64_t residues_len,
                                     const uint64_t* d_offsets, uint64_t n, const uint32_t* d_select,
                                     const uint32_t* d_select_count, float* d_bias, void* stream);
msv_status msv_bf_profile_bind_stream(msv_bf_profile* profile, void* stream);
msv_status msv_bf_profile_check(msv_bf_profile* profile, void* stream);
/* msv_filter_select_device with the bias term: the same stable compaction in d_order, the same order contract;
 * with d_bias all zero its list is msv_filter_select_device's. */
msv_status msv_bf_filter_select_device(int device, const float* d_scores, const float* d_bias,
                                       const uint64_t* d_offsets, const uint32_t* d_order, uint64_t n, float mu,
                                       float lambda, double threshold, double* d_pvalues, uint32_t* d_selected,
                                       uint32_t* d_count, void* stream);
/* msv_bf_pvalues on the device (msv_pvalues_device / msv_fwd_pvalues_device with the bias term). */
msv_status msv_bf_pvalues_device(int device, const float* d_scores, const float* d_bias, const uint64_t* d_offsets,
                                 uint64_t n, float location, float scale, int kind, double* d_pvalues, void* stream);

/* Options of msv_fwd_filter_batch_opts.  Append-only: struct_size is set by the caller to sizeof(msv_search_options);
 * fields beyond it read as 0.  NULL options are all zeros. */
typedef struct msv_search_options {
    uint64_t struct_size;
    int32_t bias_filter;          /* run the bias filter between MSV and Viterbi                     */
    int32_t reserved;
    msv_bf_profile* bias_profile; /* needed with bias_filter, on the cascade's device               */
} msv_search_options;
/* msv_fwd_filter_batch with options; msv_fwd_filter_batch is this call with NULL options, and with bias_filter = 0
 * no launch or allocation is added and every output is that call's (bias, passed_bias, n_passed_bias may then be NULL;
 * when given, bias is zeros and passed_bias is passed_msv).  With bias_filter, on one stream with no host round trip:
 * MSV over all; P <= F1 on null1 gives list A (passed_msv); the bias of list A (0 elsewhere, which reproduces a
 * sequence's null1 P-value exactly and keeps it out); filtered MSV P <= F1 gives list B (passed_bias), in the same
 * longest-first order; Viterbi on B; filtered Viterbi P <= F2 gives list C (passed_vit); Forward on C; fwd_pvalues
 * are the filtered ones (1 where Forward did not run), taken on the host after the download: msv_bf_pvalues on
 * fwd_scores and bias, to the last bit. */
msv_status msv_fwd_filter_batch_opts(msv_profile* msv, msv_vit_profile* vit, msv_fwd_profile* fwd,
                                     const uint8_t* residues, const uint64_t* offsets, uint64_t n, const float* stats,
                                     double F1, double F2, const msv_search_options* options, float* msv_scores,
                                     uint8_t* passed_msv, float* vit_scores, uint8_t* passed_vit, float* fwd_scores,
                                     double* fwd_pvalues, uint64_t* n_passed_msv, uint64_t* n_passed_vit, float* bias,
                                     uint8_t* passed_bias, uint64_t* n_passed_bias);

/* ---- Split stage: stochastic traceback ensembles and the clustering of multi-domain regions ----
 * A region that holds several tandem copies of a domain must not be rescored as one envelope.  This is the step of
 * HMMER3's p7_domaindef_ByPosteriorHeuristics between the region rule and rescore_isolated_domain: a region is
 * tested (is_multidomain_region), a multi-domain region has n_samples alignments sampled from the posterior by
 * stochastic traceback over its Forward matrix, the sampled domains are clustered by their end points
 * (p7_spensemble_Cluster) and each cluster's envelope is rescored by the alignment stage in place of the region.
 * As for every stage since Viterbi, parity with HMMER is unpinned: the model is this header's (D_k -> E exits, no
 * unihit reconfiguration for an envelope, as the alignment stage says), the random numbers are this block's.
 *
 * Which regions are split.  On the float32 begin / end arrays of msv_dom_decode_batch (residue i at index i - 1),
 * for a region i_from .. i_to: Esum(z) = the serial float sum of end[i_from .. z] accumulated upward, Bsum(z) = the
 * serial float sum of begin[z .. i_to] accumulated downward from i_to; the region is multi-domain iff
 * max_z min(Esum(z), Bsum(z)) >= rt3 (HMMER's default 0.20).  Adds and compares only.
 *
 * The matrix.  An item is the alignment stage's (an envelope of Le residues decoded as a sequence of its own with
 * the loop / move of the parent's length Lc).  A recording Forward launch (spl_kernel.hip: the Forward row of the
 * Forward, domain and alignment stages, unchanged) stores for every row i = 1..Le the three planes fM, fI, fD as
 * float32 in the scale of the row's exponent, next to the Le + 1 six-word records N, J, C, B, E, exponent of the
 * domain stage: a stored value x of row i stands for x 2^exponent(i).  Every stored f carries Forward's relative
 * bound 16 (Le + LENG) 2^-24 against msv_spl_cpu_forward (absolute 2^-126 in the row's scale where the float32
 * value is subnormal or zero).
 *
 * The sampler (msv_spl_sample is THE definition; the device's spl_sample_kernel runs the same function,
 * spl_host.h's spl_sample, one (item, sample) per thread, and reproduces it byte for byte on the same arrays).
 * The walk starts in C(Le) and draws every source, options in this order, values as stored (float32), t the
 * float32 odds of the device tables ((float) exp((double) score)), transitions indexed as in the Forward block:
 *   C(i)   : C(i-1) loop | E(i) tEC                J(i) : J(i-1) loop | E(i) tEJ            B(i) : N(i) | J(i)
 *   E(i)   : M(i,1), then for k = 2..LENG: M(i,k), D(i,k)
 *   M(i,k) : M(i-1,k-1) tMM[k-1] | I(i-1,k-1) tIM[k-1] | D(i-1,k-1) tDM[k-1] | B(i-1) tBM
 *   I(i,k) : M(i-1,k) tMI[k] | I(i-1,k) tII[k]     D(i,k) : M(i,k-1) tMD[k-1] | D(i,k-1) tDD[k-1]
 * (row 0 and node 0 hold zeros and are not read).  In the two `loop` draws the older value is first moved to the
 * newer row's scale by multiplications by powers of two (the recorded exponent difference; exact while the moved
 * value is a normal float32, correctly rounded below that).  A draw: the
 * weights w_j, each product rounded to float32 on its own; T = their float32 sum in index order; u = a 24-bit
 * integer times 2^-24; t = u T (one rounding); the first j whose running prefix sum in the same order exceeds t;
 * if none does, the last j with w_j > 0.  A weight of 0 is never picked.  T = 0 (every product underflowed) marks
 * the sample truncated: it yields no further domain and is counted in the stats.  E's draw takes two passes over
 * the row: the sum, then the pick.  No multiply feeds an add unrounded: the host object of this function is built
 * with -ffp-contract=off as the device objects are.  Picking B from M(i,k) ends a domain (i_from = i, k_from = k;
 * i_to and k_to are where E was left: k_to is the exit node, an M or a D); B(i) -> N ends the path, B(i) -> J
 * continues with J(i).  Every step lowers i or k.
 * Random numbers are counter-based, stateless and integer-only: with mix(x) the splitmix64 finaliser and
 * g = 0x9e3779b97f4a7c15, h = seed, then h = mix(h + g + v) for v = the parent's sequence index, i_from, i_to (the
 * envelope's, relative to the parent) and the sample index in turn; draw d = 0, 1, .. of the sample is
 * mix(h + g (d + 1)) >> 40.  The key is the envelope's identity, so an item's samples do not depend on the batch,
 * the item order, the chunking or the stream.  Defaults: seed 42, 200 samples (HMMER's).
 *
 * Clustering (msv_spl_cluster, host only): HMMER's single linkage on the segments (i_from, i_to, k_from, k_to) of
 * all samples of one item.  Two segments are linked iff their residue ranges overlap by at least min_overlap of
 * the shorter one, their node ranges likewise, |(i_from - k_from) - (i_from' - k_from')| <= max_diagdiff and the
 * same for (i_to - k_to).  Fractions are integer ratios num / den and every test is in integers:
 * den overlap >= num min(len, len'), with overlap = max(0, min(to, to') - max(from, from') + 1).  Clusters are the
 * connected components, numbered by their lowest segment index; a cluster of `count` segments is kept iff
 * den count >= num n_samples (min_posterior, 1/4).  Its i_from is the smallest value whose frequency f among the
 * cluster's i_from has den f >= num count (min_endpointp, 1/50), its i_to the largest such value, k_from and k_to
 * likewise (where no value reaches it, the smallest / largest value seen).  Envelopes come sorted by i_from (then
 * cluster number), each with prob = count / n_samples (float).
 * A multi-domain region is replaced by its clusters' envelopes, which may overlap; if no cluster passes, the
 * region yields none. */
typedef struct msv_spl_segment {
    uint32_t i_from, i_to;         /* residues, 1-based, relative to the parent sequence */
    uint32_t k_from, k_to;         /* nodes */
} msv_spl_segment;
typedef struct msv_spl_envelope {
    uint32_t i_from, i_to, k_from, k_to;
    uint32_t count;                /* segments of the cluster */
    float prob;                    /* count / n_samples */
} msv_spl_envelope;
/* Append-only: struct_size is set by the caller; fields beyond it read as 0 and 0 means the default. */
typedef struct msv_spl_cluster_options {
    uint64_t struct_size;
    uint32_t min_overlap_num, min_overlap_den;        /* 4 / 5  */
    uint32_t max_diagdiff;                            /* 4 (UINT32_MAX: no limit; 0 is the default, not zero) */
    uint32_t min_posterior_num, min_posterior_den;    /* 1 / 4  */
    uint32_t min_endpointp_num, min_endpointp_den;    /* 1 / 50 */
    uint32_t reserved;
} msv_spl_cluster_options;
typedef struct msv_spl_options {
    uint64_t struct_size;
    uint64_t workspace_bytes;      /* device workspace of a chunk (0 = 1 GiB)                              */
    uint64_t seed;                 /* used as given when seed_set, else 42                                 */
    uint32_t n_samples;            /* 0 = 200                                                              */
    int32_t seed_set;
    int32_t keep_matrix;           /* keep the recorded planes on the host for msv_spl_result_matrix       */
    int32_t reserved;
    void* stream;                  /* NULL: the profile's own                                              */
} msv_spl_options;
typedef struct msv_spl_result msv_spl_result;

/* The region test above; *multidomain = 0 / 1.  i_from < 1, i_from > i_to or i_to > L: MSV_ERR_INVALID_ARGUMENT. */
msv_status msv_dom_is_multidomain(const float* begin, const float* end, uint64_t L, uint32_t i_from, uint32_t i_to,
                                  float rt3, int* multidomain);
/* The float64 twin of the recording launch: the serial Forward of one envelope with D kept (rescaled by 2^256 as
 * msv_dom_cpu_decode, model arguments as msv_aln_cpu_decode).  fM, fI, fD double [Le][LENG + 1] (row i - 1, column
 * k; column 0 is 0), specials double [Le + 1][5] = N, J, C, B, E of rows 0..Le, exponents int32 [Le + 1]: a value x
 * of row i stands for x 2^exponents[i].  *score = log Z.  Any output may be NULL. */
msv_status msv_spl_cpu_forward(const float* match_scores, const float* insert_scores, const float* transition_scores,
                               uint32_t model_length, float tr_B_Mk, float tr_E_C, float tr_E_J, const uint8_t* codes,
                               uint64_t Le, uint64_t Lc, double* score, double* fM, double* fI, double* fD,
                               double* specials, int32_t* exponents);
/* THE definition of one sample, on arrays laid out as msv_spl_result_matrix returns them: fM, fI, fD float
 * [Le][LENG + 1], records uint32 [Le + 1][6].  The sample's identity (seed, seq, i_from, i_to, sample) keys its
 * random numbers; the envelope is residues i_from .. i_to of its parent (Le = i_to - i_from + 1) and segments carry
 * residues relative to the parent.  Two calls size the output: with segments NULL only the counts are written; then
 * segments[*n_segments], in residue order, and where ops is given the path as the Viterbi trace reports one:
 * domains[*n_segments] (seq = 0, residues relative to the ENVELOPE, ops_begin from 0) and ops[*n_ops].
 * *truncated = 1 if a draw met T = 0. */
msv_status msv_spl_sample(const float* fM, const float* fI, const float* fD, const uint32_t* records,
                          const float* transition_scores, uint32_t model_length, float tr_B_Mk, float tr_E_C,
                          float tr_E_J, uint64_t Lc, uint64_t seed, uint32_t seq, uint32_t i_from, uint32_t i_to,
                          uint32_t sample, uint32_t* n_segments, uint64_t* n_ops, int* truncated,
                          msv_spl_segment* segments, msv_vit_domain* domains, uint8_t* ops);
/* The clustering above on the n_segments segments of one item's n_samples samples, by the two-call protocol: with
 * envelopes NULL only *n_envelopes is written.  NULL options are the defaults. */
msv_status msv_spl_cluster(const msv_spl_segment* segments, uint64_t n_segments, uint32_t n_samples,
                           const msv_spl_cluster_options* options, uint32_t* n_envelopes,
                           msv_spl_envelope* envelopes);
/* Workspace bytes of one item under a variant of S = states_per_lane: Le + 1 six-word records and Le rows of
 * 3 S x 64 floats (fM, fI, fD by slot).  Chunks are cut by msv_vit_trace_chunk_cuts. */
uint64_t msv_spl_item_bytes(uint32_t states_per_lane, uint64_t Le);

/* Samples the items of a host batch on the device, synchronous: per chunk of items the recording launch, then the
 * sampler's count pass, a host scan and its place pass.  Items, their checks, the workspace rule and the error
 * classes are msv_aln_align_batch's; an item that was not decoded has no segments.  Results are per item in the
 * caller's order, item q's sample j at entry q n_samples + j. */
msv_status msv_spl_sample_batch(msv_dom_profile* profile, const uint8_t* residues, const uint64_t* offsets, uint64_t n,
                                const msv_aln_item* items, uint64_t n_items, const msv_spl_options* options,
                                msv_spl_result** result);
uint64_t msv_spl_result_count(const msv_spl_result* result);     /* items */
uint64_t msv_spl_result_segments(const msv_spl_result* result);  /* segments in all */
/* envelope_scores[count], sample_offsets[count n_samples + 1], segments[]; any may be NULL. */
msv_status msv_spl_result_copy(const msv_spl_result* result, float* envelope_scores, uint64_t* sample_offsets,
                               msv_spl_segment* segments);
/* Item q's recorded planes as the device wrote them (keep_matrix, else MSV_ERR_INVALID_ARGUMENT), for tests: fM, fI,
 * fD float [Le][LENG + 1], records uint32 [Le + 1][6]; any may be NULL.  An item that was not decoded has zeros. */
msv_status msv_spl_result_matrix(const msv_spl_result* result, uint64_t q, float* fM, float* fI, float* fD,
                                 uint32_t* records);
/* Append-only, as msv_aln_null2_stats. */
typedef struct msv_spl_stats {
    uint32_t struct_size;
    uint32_t n_samples;
    uint64_t seed;
    uint64_t chunks;
    uint64_t matrix_bytes;         /* the recording launches wrote                  */
    uint64_t truncated;            /* samples that met T = 0                        */
    float forward_ms, sample_ms;   /* summed device times (HIP events); the sampler's two passes together */
} msv_spl_stats;
msv_status msv_spl_result_stats(const msv_spl_result* result, msv_spl_stats* out);
void msv_spl_result_free(msv_spl_result* result);
/* Append-only, as msv_aln_info. */
typedef struct msv_spl_info {
    uint32_t struct_size;
    uint32_t states_per_lane;
    uint32_t forward_blocks;
    uint32_t forward_scratch_bytes, sample_scratch_bytes;
    uint32_t forward_lds_bytes, sample_lds_bytes;
    uint32_t reserved;
    uint64_t default_workspace_bytes;
    char variant[64];
} msv_spl_info;
msv_status msv_spl_describe(const msv_dom_profile* profile, msv_spl_info* out);

/* ---- Calibration: the engines' own mu, tau and lambda ------------------------------------------
 * Every P-value of this library goes through the three pairs STATS LOCAL MSV / VITERBI / FORWARD of the .hmm file,
 * which hmmbuild fitted to HMMER3's own 8-bit and 16-bit filters, not to this library's float engines.  This block
 * restates HMMER3's p7_Calibrate for the engines here: a null sample is generated, scored by the engines and
 * fitted, all on the device.  As for every stage since Viterbi, parity with HMMER is unpinned.  The file's own
 * statistics are never modified: the fitted six are returned, and the cascade takes them in place of the file's.
 *
 * Lambda (p7_Lambda), float64: H = (1 / LENG) sum_k sum_x p_k[x] log2(p_k[x] / f[x]) over the parsed match
 * emissions of nodes 1..LENG (terms with p = 0 are 0) and the background f; lambda = ln 2 + 1.44 / (LENG H).
 *
 * The null sample.  Residue i (0-based) of sequence s of sample set `set` (0 MSV, 1 Viterbi, 2 Forward) under `seed`:
 * with mix and g of the split stage's random numbers, h = seed, h = mix(h + g + set), h = mix(h + g + s);
 * u = mix(h + g (i + 1)) >> 40 (24 bits); code = the number of j in 0..18 with u >= T[j], where
 * T[j] = (uint32) floor(2^24 (f[0] + .. + f[j]) / (f[0] + .. + f[19])), the sums in float64 in index order.
 * Integers only and no state: any slice of any chunk is reproducible.  msv_cal_generate is THE definition; the
 * device kernel's bytes equal it.
 *
 * The fits, float64 over float32 bit scores x_i = bits_of(score_i - nullsc(L)) (the float expressions of
 * msv_pvalues; L = 0 means the scores ARE bit scores and are taken as they are).  y_i = x_i - x_min.
 *   location at fixed lambda (esl_gumbel_FitCompleteLoc; MSV, Viterbi):
 *       mu = x_min - log((1 / n) sum_i exp(-lambda y_i)) / lambda
 *   complete fit (esl_gumbel_FitComplete; Forward): lambda0 = pi / sqrt(6 var), var = sum (y_i - ybar)^2 / (n - 1);
 *       Newton on f(l) = 1 / l - ybar + S1 / S0, f'(l) = (S1 / S0)^2 - S2 / S0 - 1 / l^2, S_p = sum y_i^p exp(-l y_i):
 *       each iteration evaluates (f, f') at l, takes step = f / f', moves to l - step (or to l / 2 where that is
 *       <= 0) and stops when |step| <= 1e-9 l; after 100 iterations without that, MSV_ERR_NO_CONVERGENCE (also for a
 *       lambda that stops being finite).  There is no fallback.  mu is the location formula at the final lambda.
 *   tau (p7_Tau): tau = gmu - log(-log(1 - t)) / glam + log(t) / lambda_profile, (gmu, glam) the complete fit,
 *       t the tail mass (default 0.04).
 * n < 2, all scores equal (zero variance), a bit score that is not finite, lambda <= 0 or a tail outside (0, 1):
 * MSV_ERR_INVALID_ARGUMENT.  Order of summation, fixed: the host adds in index order; the device kernel (one
 * workgroup of 256 threads) has thread t add elements t, t + 256, .. in index order and then halves an LDS tree
 * (t += t + 128, 64, .., 1).  Neither depends on the run.  DESIGN 4.15 derives the bounds between the two. */
enum { MSV_CAL_SET_MSV = 0, MSV_CAL_SET_VITERBI = 1, MSV_CAL_SET_FORWARD = 2 };
typedef enum msv_cal_fit_mode {
    MSV_CAL_FIT_LOCATION = 0, /* mu at the given lambda                                         */
    MSV_CAL_FIT_GUMBEL = 1,   /* the complete fit: (mu, lambda)                                 */
    MSV_CAL_FIT_TAU = 2       /* the complete fit, then tau at the given lambda and tail        */
} msv_cal_fit_mode;
/* The record the fit kernel writes (40 bytes).  LOCATION: mu, lambda as given (gmu, glam repeat them).  GUMBEL:
 * mu = gmu, lambda = glam.  TAU: mu = tau, lambda as given, (gmu, glam) the fitted Gumbel.  status is a msv_status;
 * where it is not MSV_OK the four doubles are NaN. */
typedef struct msv_cal_fit {
    double mu, lambda, gmu, glam;
    uint32_t iterations;      /* Newton iterations (0 for LOCATION) */
    uint32_t status;
} msv_cal_fit;
/* Append-only: struct_size is set by the caller; fields beyond it read as 0 and 0 means the default.  Index = set. */
typedef struct msv_cal_options {
    uint64_t struct_size;
    uint64_t n[3];            /* sequences: HMMER's 200, 200, 200                                          */
    uint64_t length[3];       /* their length: HMMER's 200, 200, 100                                       */
    double tail;              /* tail mass of tau: 0.04                                                    */
    uint64_t seed;            /* used as given when seed_set, else 42                                      */
    int32_t seed_set;
    int32_t insert_mode;      /* msv_cal_cpu_calibrate only: the engines' (the device call's engines hold theirs) */
    uint64_t workspace_bytes; /* device bytes of a chunk's residues and offsets (0 = 256 MiB)              */
    float* scores[3];         /* optional host arrays of n[set] floats: the set's raw scores (nats), copied out
                                 after the fit for tests and tools                                         */
} msv_cal_options;
/* Append-only, struct_size set by the caller. */
typedef struct msv_cal_report {
    uint32_t struct_size;
    uint32_t ran;             /* bit s: set s was run                                                      */
    double lambda;            /* the profile's (msv_cal_lambda)                                            */
    double location[3];       /* MSV mu, Viterbi mu, Forward tau (NaN where not run)                       */
    double gmu, glam;         /* the Gumbel fitted to the Forward sample                                   */
    uint32_t iterations;      /* of that fit's Newton loop                                                 */
    uint32_t reserved;
    uint64_t chunks[3];       /* generate + score launches per set                                         */
    uint64_t n[3], length[3]; /* as run                                                                    */
    uint64_t seed;
    double tail;
} msv_cal_report;

/* Host-only.  match_emissions: [model_length][20] as msv_hmm_match_emissions (row 0 is the dummy node). */
msv_status msv_cal_lambda(const float* match_emissions, uint32_t model_length, const float* background,
                          double* lambda);
/* The 19 thresholds T of the null sample, and the codes of n given 24-bit draws (the count rule above). */
msv_status msv_cal_thresholds(const float* background, uint32_t* thresholds);
msv_status msv_cal_codes_of_draws(const float* background, const uint32_t* draws, uint64_t n, uint8_t* codes);
/* THE definition of the null sample: sequences first .. first + n - 1 of `set`, each of L residues, as a CSR batch:
 * codes[n L], offsets[n + 1] = 0, L, 2 L, ..  L must be below 2^32 - 1. */
msv_status msv_cal_generate(const float* background, uint64_t seed, uint32_t set, uint64_t first, uint64_t n,
                            uint64_t L, uint8_t* codes, uint64_t* offsets);
msv_status msv_cal_fit_location(const float* scores, uint64_t n, uint64_t L, double lambda, double* mu);
msv_status msv_cal_fit_gumbel(const float* scores, uint64_t n, uint64_t L, double* mu, double* lambda,
                              uint32_t* iterations);
msv_status msv_cal_tau(double gmu, double glam, double lambda, double tail, double* tau);
/* The CPU twin of msv_cal_calibrate: the same sample from msv_cal_generate, scored by the CPU paths (the MSV DP
 * of MSV_HMM::run_on_sequence, msv_vit_cpu_score's, msv_fwd_cpu_score_batch rounded to float) and fitted on the
 * host.  sets: bit s runs set s; the others' slots of stats stay as the caller filled them. */
msv_status msv_cal_cpu_calibrate(const msv_hmm* hmm, uint32_t sets, const msv_cal_options* options, float* stats,
                                 msv_cal_report* report);

/* Device bytes of a chunk of n sequences of length L: the codes rounded up to 16 bytes, then n + 1 offsets. */
uint64_t msv_cal_workspace_bytes(uint64_t n, uint64_t L);
/* msv_cal_generate on the device, enqueued on `stream` (a hipStream_t; not NULL): one thread writes 16
 * consecutive code bytes with one vector store (the ragged end in byte stores), the same launch the offsets.
 * d_codes must be 16-byte aligned with room for n L bytes, n L < 2^32 - 2^20. */
msv_status msv_cal_generate_device(int device, const float* background, uint64_t seed, uint32_t set, uint64_t first,
                                   uint64_t n, uint64_t L, uint8_t* d_codes, uint64_t* d_offsets, void* stream);
/* One fit launch (a single workgroup) over n device scores; writes *d_record.  Nothing is read back: the record's
 * status word carries the fit's errors. */
msv_status msv_cal_fit_device(int device, const float* d_scores, uint64_t n, uint64_t L, int mode, double lambda,
                              double tail, msv_cal_fit* d_record, void* stream);
/* The stage.  Per engine that is not NULL: the set's N sequences are generated in chunks that fit the workspace
 * (and the engines' limit of 2^32 - 2^20 residue bytes per call), each chunk scored by the engine's device call
 * into the set's N-float array, then one fit launch; nothing crosses PCIe between the seed and the result record.
 * On its own stream; the engines' length tables are reserved for L and their latched errors returned through
 * their check calls.  stats: msv_hmm_stats' six; a NULL engine leaves its two slots as the caller filled them;
 * each lambda slot written is the profile's lambda.  report may be NULL.  The engines must live on one device. */
msv_status msv_cal_calibrate(const msv_hmm* hmm, msv_profile* msv, msv_vit_profile* vit, msv_fwd_profile* fwd,
                             const msv_cal_options* options, float* stats, msv_cal_report* report);

/* ---- Emit stage: sequences drawn from the profile, with their true paths ------------------------
 * The positive sample, the sibling of calibration's null sample: the scoring model of the stages above run FORWARDS
 * over the parsed probabilities (msv_hmm_match_emissions, msv_hmm_insert_emissions, msv_hmm_transitions, the
 * background), on the device, into a CSR batch the engines' *_device calls take as it is, with each sequence's true
 * domains and 'M' / 'I' / 'D' ops in the layout of the Viterbi traces (domain_offsets, msv_vit_domain, ops).
 * This samples THIS LIBRARY's model: a fragment (k_start, k_end) is uniform over the LENG (LENG + 1) / 2 pairs -- the
 * implicit local model a constant tr_B_Mk with free exits stands for -- not HMMER's occupancy-weighted entry, so
 * parity with hmmemit / p7_ProfileEmit is unpinned, like every stage since Viterbi.
 *
 * Configuration: a configured length Lc (loop = Lc / (Lc + 3), move = 3 / (Lc + 3): the probabilities behind
 * msv_sequence_transitions(Lc); Lc = 0 is legal and gives no flanks); multihit (E -> J with 1/2, E -> C with 1/2, the
 * engines' nu = 2) or unihit (E -> C always, no draw); the insert mode (MSV_INSERTS_ZERO: insert residues from the
 * background, as the engines score them; MSV_INSERTS_LOG_ODDS: from the file's insert emissions); max_length.
 *
 * The walk.  N: while a draw says loop, emit a residue from the background; then B.  B draws a fragment, 1 <= k_start
 * <= k_end <= LENG; the core starts in M(k_start).  M(k) emits from match row k and, at k < k_end, draws among
 * tMM / tMI / tMD of node k (to M(k+1), I(k), D(k+1)); I(k) emits, then draws tIM / tII (to M(k+1), I(k)); D(k) at
 * k < k_end draws tDM / tDD (to M(k+1), D(k+1)); M(k_end) or D(k_end) goes to E (D -> E exits are the Forward
 * model's).  Only transitions of nodes 1 .. LENG-1 are read, the Viterbi stage's rule, so no '*' entry is touched.
 * E draws J or C (multihit).  J behaves as N, then B again; C behaves as N, then the walk ends.
 *
 * Integers only.  A categorical draw over weights w[0..c) compares a 24-bit draw u with the c - 1 thresholds
 * T[j] = (uint32) floor(2^24 (w[0] + .. + w[j]) / (w[0] + .. + w[c-1])), float64 sums in index order (the count rule
 * of msv_cal_thresholds): the category is the number of j with u >= T[j].  Groups, in this category order: loop /
 * move; J / C; the 20 residues of the background, of a match row, of an insert row; MM / MI / MD, IM / II, DM / DD of
 * a node.  A group whose total is not positive and finite gives MSV_ERR_INVALID_ARGUMENT when the tables are built.
 * The fragment is a 32-bit draw r: index (r npairs) >> 32 into the pairs ordered by k_start, then k_end, decoded by
 * an integer binary search over the cumulative counts C(s) = (s - 1) LENG - (s - 1)(s - 2) / 2 of the pairs before
 * k_start = s.  Keys, with mix and g of the split stage's random numbers: h = seed, h = mix(h + g + MSV_EMIT_STREAM),
 * h = mix(h + g + s) for sequence index s; draw d = 0, 1, .. of the walk, in the order the walk makes them, is
 * mix(h + g (d + 1)) >> 40 (24 bits) or >> 32 (32 bits).  MSV_EMIT_STREAM is no sample set of calibration, so no
 * key is shared with it.  A sequence depends on (seed, s, the configuration) and on nothing else.
 *
 * max_length: when the walk has emitted max_length residues it stops where it stands; an open domain is closed at
 * the current node (so a truncated domain's last op may be 'I') and the sequence is flagged truncated.
 *
 * Truth.  Per sequence its domains (i_from, i_to: the first and last residue the domain emitted; k_from = k_start,
 * k_to the exit node), one op byte per core state in path order; residues outside domains come from N, J, C.
 * msv_emit_generate is THE definition; the device bytes equal it. */
#define MSV_EMIT_STREAM 0x454d4954u /* "EMIT" */
/* Append-only: struct_size is set by the caller; fields beyond it read as 0. */
typedef struct msv_emit_options {
    uint64_t struct_size;
    uint64_t length;          /* Lc, as given when length_set (0 is legal), else 400                        */
    uint64_t max_length;      /* 0 = the default, 2^20; at most 2^31 - 1                                    */
    int32_t length_set;
    int32_t unihit;           /* 0 multihit, 1 unihit                                                       */
    int32_t insert_mode;      /* msv_insert_mode                                                            */
    int32_t reserved;
} msv_emit_options;
/* The record the scan launch writes and the host reads back. */
typedef struct msv_emit_totals {
    uint64_t residues, domains, ops, truncated;
    uint64_t overflow;        /* bit 0 residues, 1 domains, 2 ops: that total exceeds its capacity         */
} msv_emit_totals;
/* The truth buffers of a device call (device pointers; capacities in elements). */
typedef struct msv_emit_truth {
    uint64_t* d_domain_offsets;   /* [n + 1]                                                                */
    msv_vit_domain* d_domains;    /* seq = index within the call, ops_begin into d_ops                      */
    uint64_t domains_capacity;
    uint8_t* d_ops;
    uint64_t ops_capacity;
    uint8_t* d_truncated;         /* [n] 0 / 1                                                              */
} msv_emit_truth;
typedef struct msv_emit_result msv_emit_result;
typedef struct msv_emit_profile msv_emit_profile;

/* Host-only.  The integer tables: background[19], match[model_length][19] and insert[model_length][19] (row 0 and,
 * for the inserts, every row outside 1 .. LENG-1 are zeros; under MSV_INSERTS_ZERO the insert rows repeat the
 * background's), transitions[model_length][4] = (T_MM, T_MM+MI, T_IM, T_DM) of nodes 1 .. LENG-1 (zeros elsewhere),
 * specials[2] = (T_loop, T_J; T_J = 0 for unihit).  Any output may be NULL. */
msv_status msv_emit_tables(const msv_hmm* hmm, const msv_emit_options* options, uint32_t* background, uint32_t* match,
                           uint32_t* insert, uint32_t* transitions, uint32_t* specials);
/* THE definition: sequences first .. first + n - 1 under `seed`. */
msv_status msv_emit_generate(const msv_hmm* hmm, const msv_emit_options* options, uint64_t seed, uint64_t first,
                             uint64_t n, msv_emit_result** result);
uint64_t msv_emit_result_count(const msv_emit_result* result);     /* sequences */
uint64_t msv_emit_result_residues(const msv_emit_result* result);
uint64_t msv_emit_result_domains(const msv_emit_result* result);
uint64_t msv_emit_result_ops(const msv_emit_result* result);
uint64_t msv_emit_result_chunks(const msv_emit_result* result);    /* device chunks (0 for the host definition) */
/* codes[residues], offsets[count + 1], domain_offsets[count + 1], domains[] (seq = index in the result), ops[],
 * truncated[count]; any may be NULL.  A result made without truth has no domains and no ops. */
msv_status msv_emit_result_copy(const msv_emit_result* result, uint8_t* codes, uint64_t* offsets,
                                uint64_t* domain_offsets, msv_vit_domain* domains, uint8_t* ops, uint8_t* truncated);
void msv_emit_result_free(msv_emit_result* result);
/* The score in nats (float64 sums of the engines' float32 tables, msv_hmm_viterbi_scores' layout; insert_scores NULL =
 * zeros) of the given true path of one sequence of L residues under msv_sequence_transitions(L): every residue
 * outside the domains costs tr_loop, N -> B, every J -> B and the final C move cost tr_move, every domain tr_B_Mk,
 * its emissions and transitions (the exit is free) and tr_E_J (tr_E_C for the last).  -inf for a path without
 * domains (the scoring model has none); MSV_ERR_INVALID_ARGUMENT for ops that do not replay from (i_from, k_from)
 * to (i_to, k_to) inside the sequence and the model, or domains that overlap. */
msv_status msv_emit_path_score(const float* match_scores, const float* insert_scores, const float* transition_scores,
                               uint32_t model_length, float tr_B_Mk, float tr_E_C, float tr_E_J, const uint8_t* codes,
                               uint64_t L, const msv_vit_domain* domains, uint32_t n_domains, const uint8_t* ops,
                               double* score);
/* Device bytes of one chunk of n sequences holding these totals (msv_emit_batch's workspace arithmetic): 16 n bytes
 * of counts, n + 1 offsets, then -- with truth -- n + 1 domain offsets and n flags, then the codes, the domains and
 * the ops, each part rounded up to 16 bytes. */
uint64_t msv_emit_workspace_bytes(uint64_t n, uint64_t residues, uint64_t domains, uint64_t ops, int truth);

/* The device handle: the threshold tables, uploaded once (under 400 KiB at LENG 2,432; read-only, L2-resident).
 * Threading as msv_profile: one host thread at a time. */
msv_status msv_emit_profile_create(int device, const msv_hmm* hmm, const msv_emit_options* options,
                                   msv_emit_profile** out);
void msv_emit_profile_destroy(msv_emit_profile* profile);
/* The working stream of msv_emit_batch where its `stream` is NULL (NULL unbinds: the handle's own stream). */
msv_status msv_emit_profile_bind_stream(msv_emit_profile* profile, void* stream);
/* One call, three launches on `stream` (a hipStream_t; not NULL), then the stream is waited for and *totals (may be
 * NULL) read back.  Count: one sequence per thread walks and writes (length, domains, ops, truncated).  Scan: one
 * workgroup turns the counts into the n + 1 uint64 offsets at d_offsets (and truth->d_domain_offsets) and writes the
 * totals record.  Place: the same walk with the same counters stores the codes (and domains, ops, flags).  A total
 * above its capacity: MSV_ERR_OUT_OF_MEMORY, and neither the scan nor the place launch writes any caller buffer.
 * truth NULL: only codes and offsets.  d_codes with room for `capacity` bytes; a call addresses fewer than 2^32 - 2^20
 * residue bytes (else MSV_ERR_OUT_OF_MEMORY, as a capacity).  The batch is usable by msv_score_batch_device,
 * msv_vit_*, msv_fwd_* and msv_bf_* device calls as it is. */
msv_status msv_emit_batch_device(msv_emit_profile* profile, uint64_t seed, uint64_t first, uint64_t n,
                                 uint8_t* d_codes, uint64_t capacity, uint64_t* d_offsets,
                                 const msv_emit_truth* truth, msv_emit_totals* totals, void* stream);
/* Host result of sequences first .. first + n - 1, in chunks that fit workspace_bytes (0 = 256 MiB) by
 * msv_emit_workspace_bytes: a chunk is counted and scanned, halved until it fits (a single sequence that does not:
 * MSV_ERR_OUT_OF_MEMORY), placed and downloaded.  The bytes do not depend on the chunking. */
msv_status msv_emit_batch(msv_emit_profile* profile, uint64_t seed, uint64_t first, uint64_t n, int truth,
                          uint64_t workspace_bytes, void* stream, msv_emit_result** result);
/* Device times (ms, HIP events around the launches) of the last msv_emit_batch_device or msv_emit_batch call of this
 * handle: the count, the scan and the place launch, each summed over the call's chunks and retries.  Each interval is
 * between an event recorded directly before the launch and one directly after it, so it is that kernel's time and
 * holds no copy, allocation or host wait.  Any may be NULL. */
msv_status msv_emit_profile_times(const msv_emit_profile* profile, float* count_ms, float* scan_ms, float* place_ms);
/* Append-only, struct_size set by the caller. */
typedef struct msv_emit_info {
    uint32_t struct_size;
    uint32_t model_length;
    uint32_t block;                 /* threads per workgroup of the walk kernels                            */
    uint32_t scan_block;
    uint32_t count_vgprs, place_vgprs, scan_vgprs;
    uint32_t count_scratch_bytes, place_scratch_bytes, scan_scratch_bytes;
    uint32_t count_lds_bytes, place_lds_bytes, scan_lds_bytes;
    int device;
    uint64_t table_bytes;
    uint64_t length, max_length;
    int32_t unihit, insert_mode;
    uint64_t default_workspace_bytes;
} msv_emit_info;
msv_status msv_emit_describe(const msv_emit_profile* profile, msv_emit_info* out);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* MSV_H_ */
