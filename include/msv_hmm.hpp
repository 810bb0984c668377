// msv_hmm.hpp -- C++ host surface of the MI355X MSV engine, mirroring the reference classes
// (drop-in names, argument meaning and layouts) on top of the C-ABI in msv.h:
//
//   Profile_HMM               data_readers/Profile_HMM.hpp:21-49
//   FASTA_protein_sequences   data_readers/FASTA_protein_sequences.hpp:9-14
//   MSV_HMM                   algorithms/MSV_HMM.hpp:17-44
//   Viterbi_HMM               (new) the Viterbi stage over the parts of Profile_HMM the
//                             reference parses and never scores with (Profile_HMM.cpp:107-120)
//
// Differences from the reference, all deliberate:
//   * errors throw (msv_error, or std::out_of_range for a residue outside the 20 amino acids,
//     exactly what the reference's amino_acid_num.at throws, MSV_HMM.cpp:101) instead of printing
//     and continuing with a half-built object (Profile_HMM.cpp:50-53, MSV_HMM.cpp:198-203);
//   * run_on_sequence is, as in the reference, the sequential CPU DP (this library's own
//     restatement, two rolling rows); parallel_run_on_sequence and score_batch* score on the GPU.
//     Both are bit-identical to the reference's CPU DP, so the reference's seq-vs-par differential
//     (test_MSV.cpp:23-26) compares CPU and GPU;
//   * score_batch adds the batch API the reference lacks: one kernel launch per batch.
#pragma once

#include <array>
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "msv.h"

constexpr int NUM_OF_AMINO_ACIDS = 20;
constexpr int NUM_OF_TRANSITIONS = 7;

using Probability = float;
using Profile_name = std::string;
template <int N>
using Probabilities_array = std::array<Probability, N>;
template <int N>
using Probabilities_arrays_vector = std::vector<Probabilities_array<N>>;

using Protein_sequence = std::string;  // '#' sentinel + residues, as the reference
using Protein_sequences = std::vector<Protein_sequence>;
using Log_score = float;

class msv_error : public std::runtime_error {
  public:
    msv_error(msv_status s, const std::string& what) : std::runtime_error(what), status(s) {}
    msv_status status;
};

class Profile_HMM {
  public:
    explicit Profile_HMM(const std::string& file_path);

    Profile_name name;
    Probabilities_arrays_vector<NUM_OF_AMINO_ACIDS> match_emissions;
    Probabilities_arrays_vector<NUM_OF_AMINO_ACIDS> insert_emissions;
    Probabilities_arrays_vector<NUM_OF_TRANSITIONS> transitions;
    size_t model_length = 0;

    float stats_local_msv_mu = 0, stats_local_msv_lambda = 0;
    float stats_local_viterbi_mu = 0, stats_local_viterbi_lambda = 0;
    float stats_local_forward_theta = 0, stats_local_forward_lambda = 0;
    // (The reference's members and nothing else: the constructor lives in the library and fills the caller's
    // object, so a member added here would overrun the object of every caller built against an earlier header.
    // The COMPO line is profile_compo(), below.)
};

// The COMPO line of a profile file: the model's average match composition, exp(-value) as every other row (the
// bias filter's second state emits it, msv.h "Bias filter").  It is not a member of Profile_HMM, whose layout is
// the reference's; it is read from the file through the C-ABI (msv_hmm_read, msv_hmm_compo).
inline Probabilities_array<NUM_OF_AMINO_ACIDS> profile_compo(const std::string& file_path) {
    msv_hmm* h = nullptr;
    const msv_status s = msv_hmm_read(file_path.c_str(), &h);
    if (s != MSV_OK) throw msv_error(s, std::string(msv_status_string(s)) + ": " + file_path);
    Probabilities_array<NUM_OF_AMINO_ACIDS> compo{};
    const float* c = msv_hmm_compo(h);
    for (int x = 0; x < NUM_OF_AMINO_ACIDS; ++x) compo[x] = c[x];
    msv_hmm_destroy(h);
    return compo;
}

// Residues packed for the device: codes 0..19 (255 = a symbol the scorer rejects), CSR offsets.
struct Packed_sequences {
    std::vector<uint8_t> codes;
    std::vector<uint64_t> offsets{0};
    size_t size() const { return offsets.size() - 1; }
    // '#'-prefixed strings -> codes; throws std::out_of_range on a symbol outside the 20
    static Packed_sequences pack(const Protein_sequences& seqs);
};

class FASTA_protein_sequences {
  public:
    explicit FASTA_protein_sequences(const std::string& file_path);

    Protein_sequences sequences;  // same records as the reference parser, '#'-prefixed
    Packed_sequences packed;      // the same records as device-ready codes
    std::vector<std::string> headers;
    size_t rejected = 0;
};

// A FASTA file parsed on the GPU (msv_fasta_read_device): the same records, left in device memory.
class FASTA_device {
  public:
    explicit FASTA_device(const std::string& file_path, int device = 0);
    ~FASTA_device();
    FASTA_device(const FASTA_device&) = delete;
    FASTA_device& operator=(const FASTA_device&) = delete;
    size_t size() const { return msv_fasta_device_count(handle_); }
    size_t rejected() const { return msv_fasta_device_rejected(handle_); }
    const msv_fasta_device* handle() const { return handle_; }

  private:
    msv_fasta_device* handle_ = nullptr;
};

class MSV_HMM {
  public:
    explicit MSV_HMM(const Profile_HMM& base_hmm, int device = 0);
    ~MSV_HMM();
    MSV_HMM(const MSV_HMM&) = delete;
    MSV_HMM& operator=(const MSV_HMM&) = delete;
    MSV_HMM(MSV_HMM&& o) noexcept;
    MSV_HMM& operator=(MSV_HMM&& o) noexcept;

    // One sequence ('#' + residues).  run_on_sequence: the sequential CPU DP (MSV_HMM.cpp:74-113);
    // parallel_run_on_sequence: the fused gfx950 kernel, as a batch of one (MSV_HMM.cpp:269-430).
    Log_score run_on_sequence(const Protein_sequence& seq);
    Log_score parallel_run_on_sequence(const Protein_sequence& seq, bool should_specialize = false);

    // The batch hot path: one launch for the whole set.
    std::vector<Log_score> score_batch(const Protein_sequences& seqs);
    std::vector<Log_score> score_batch(const Packed_sequences& packed);
    std::vector<Log_score> score_batch(const uint8_t* codes, const uint64_t* offsets, size_t n);
    std::vector<Log_score> score_batch(const FASTA_device& fasta);  // GPU-parsed, scored in place

    // Profiles x sequences grid (benchmark_MSV.cpp:12-24,31-41 as one call): result[p][s].
    static std::vector<std::vector<Log_score>> score_grid(const std::vector<MSV_HMM*>& profiles,
                                                          const Protein_sequences& seqs);
    // One batch sharded over several devices (profiles[k] = this model on device k), input order.
    static std::vector<Log_score> score_batch_multi(const std::vector<MSV_HMM*>& per_device,
                                                    const Protein_sequences& seqs);

    // One batch over several devices of this process, scores gathered over RCCL (msv_multi_*).
    class Multi_device;

    msv_profile* handle() { return profile_; }
    size_t model_length() const { return model_length_; }
    const std::vector<float>& emission_scores() const { return emission_scores_; }
    float tr_B_Mk() const { return tr_B_Mk_; }
    float tr_E_C() const { return tr_E_C_; }
    float tr_E_J() const { return tr_E_J_; }

  private:
    size_t model_length_ = 0;
    std::vector<float> emission_scores_;  // [20][model_length], MSV_HMM.hpp:27-28
    float tr_B_Mk_ = 0, tr_E_C_ = 0, tr_E_J_ = 0;
    msv_profile* profile_ = nullptr;
};

// MSV_HMM::Multi_device: the same model on DISTINCT devices (per_device[k] on device k), one RCCL
// communicator per device; score_batch shards the batch by residues and gathers the scores on the
// first device over RCCL (msv_multi_create / msv_multi_score_batch).  Holds the MSV_HMMs by pointer.
class MSV_HMM::Multi_device {
  public:
    explicit Multi_device(const std::vector<MSV_HMM*>& per_device);
    ~Multi_device();
    Multi_device(const Multi_device&) = delete;
    Multi_device& operator=(const Multi_device&) = delete;
    std::vector<Log_score> score_batch(const Protein_sequences& seqs);
    std::vector<Log_score> score_batch(const Packed_sequences& packed);

  private:
    msv_multi* multi_ = nullptr;
};

// The Viterbi stage (recurrence and conventions in msv.h): HMMER3's generic local Viterbi over
// the reference's parse -- insert emissions and the 7 transitions per node -- with the MSV path's specials.
// Same shape as MSV_HMM: run_on_sequence is this library's serial CPU DP, parallel_run_on_sequence and
// score_batch the gfx950 kernel (bit-identical to each other).  STATS LOCAL VITERBI gives the P-values.
// One optimal state path per traced sequence (msv.h "Viterbi traces"): entry q's domains are
// domains[domain_offsets[q] .. domain_offsets[q + 1]), a domain's ops are ops[ops_begin .. ops_begin + ops_len).
struct Viterbi_traces {
    std::vector<Log_score> scores;
    std::vector<uint64_t> domain_offsets{0};
    std::vector<msv_vit_domain> domains;
    std::vector<uint8_t> ops;
    size_t size() const { return scores.size(); }
};

class Viterbi_HMM {
  public:
    explicit Viterbi_HMM(const Profile_HMM& base_hmm, int device = 0, msv_insert_mode inserts = MSV_INSERTS_ZERO);
    ~Viterbi_HMM();
    Viterbi_HMM(const Viterbi_HMM&) = delete;
    Viterbi_HMM& operator=(const Viterbi_HMM&) = delete;
    Viterbi_HMM(Viterbi_HMM&& o) noexcept;
    Viterbi_HMM& operator=(Viterbi_HMM&& o) noexcept;

    Log_score run_on_sequence(const Protein_sequence& seq);
    Log_score parallel_run_on_sequence(const Protein_sequence& seq);
    std::vector<Log_score> score_batch(const Protein_sequences& seqs);
    std::vector<Log_score> score_batch(const Packed_sequences& packed);
    // Traces of the selected sequences (every sequence when `select` is empty and `all` is set), computed on the
    // GPU (msv_vit_trace_batch); trace_on_sequence is the serial CPU trace (msv_vit_cpu_trace), the same path.
    Viterbi_traces trace_batch(const Packed_sequences& packed, const std::vector<uint32_t>& select = {},
                               bool all = true, uint64_t workspace_bytes = 0);
    Viterbi_traces trace_on_sequence(const Protein_sequence& seq);

    msv_vit_profile* handle() { return profile_; }
    size_t model_length() const { return model_length_; }
    float viterbi_mu = 0, viterbi_lambda = 0;  // STATS LOCAL VITERBI (Profile_HMM.cpp:86-87)

  private:
    size_t model_length_ = 0;
    bool inserts_ = false;
    std::vector<float> match_scores_, insert_scores_, transition_scores_;  // [20][M], [20][M], [M][7]
    float tr_B_Mk_ = 0, tr_E_C_ = 0, tr_E_J_ = 0;
    msv_vit_profile* profile_ = nullptr;
};

// HMMER3's filter cascade on the GPU (msv_vit_filter_batch): MSV scores of every sequence, the survivors of
// P <= F1 against (msv_mu, msv_lambda) -- a Profile_HMM's stats_local_msv_mu/lambda -- and their Viterbi
// scores (-inf where a sequence did not pass).
struct Filter_result {
    std::vector<Log_score> msv_scores;
    std::vector<uint8_t> passed;
    std::vector<Log_score> viterbi_scores;
    size_t n_passed = 0;
};
Filter_result filter_pipeline(MSV_HMM& msv, Viterbi_HMM& vit, const Packed_sequences& packed, float msv_mu,
                              float msv_lambda, double F1 = 0.02);

// The Forward stage (msv.h "Forward stage"): the log of the summed odds of every alignment, in nats.
// run_on_sequence is the library's serial float64 CPU Forward, the reference of every test;
// parallel_run_on_sequence and score_batch the gfx950 kernel (float32 odds, within msv.h's tolerance of it).
// STATS LOCAL FORWARD gives the P-values.
class Forward_HMM {
  public:
    explicit Forward_HMM(const Profile_HMM& base_hmm, int device = 0, msv_insert_mode inserts = MSV_INSERTS_ZERO);
    ~Forward_HMM();
    Forward_HMM(const Forward_HMM&) = delete;
    Forward_HMM& operator=(const Forward_HMM&) = delete;

    double run_on_sequence(const Protein_sequence& seq);
    Log_score parallel_run_on_sequence(const Protein_sequence& seq);
    std::vector<Log_score> score_batch(const Protein_sequences& seqs);
    std::vector<Log_score> score_batch(const Packed_sequences& packed);
    std::vector<double> pvalues(const std::vector<Log_score>& scores, const Packed_sequences& packed) const;

    msv_fwd_profile* handle() { return profile_; }
    size_t model_length() const { return model_length_; }
    float forward_tau = 0, forward_lambda = 0;  // STATS LOCAL FORWARD

  private:
    size_t model_length_ = 0;
    bool inserts_ = false;
    std::vector<float> match_scores_, insert_scores_, transition_scores_;  // [20][M], [20][M], [M][7]
    float tr_B_Mk_ = 0, tr_E_C_ = 0, tr_E_J_ = 0;
    msv_fwd_profile* profile_ = nullptr;
};

// HMMER3's whole cascade on the GPU (msv_fwd_filter_batch): MSV -> P <= F1 -> Viterbi -> P <= F2 -> Forward ->
// P-value, with the six STATS values of the profile (msv mu, lambda, viterbi mu, lambda, forward tau, lambda).
struct Search_result {
    std::vector<Log_score> msv_scores, viterbi_scores, forward_scores;  // -inf where a stage did not run
    std::vector<uint8_t> passed_msv, passed_viterbi;
    std::vector<double> forward_pvalues;
    size_t n_passed_msv = 0, n_passed_viterbi = 0;
};
Search_result search_pipeline(MSV_HMM& msv, Viterbi_HMM& vit, Forward_HMM& fwd, const Packed_sequences& packed,
                              const Profile_HMM& stats, double F1 = 0.02, double F2 = 1e-3);

// The domain stage (msv.h "Domain stage"): Backward, the per-residue domain posteriors and the
// envelopes of each selected sequence, on the GPU (decode_batch) or by the float64 CPU twin (decode_on_sequence).
// Per select entry q: scores [q], posteriors [residue_offsets[q], residue_offsets[q+1]), regions
// [region_offsets[q], region_offsets[q+1]).
struct Envelopes {
    std::vector<Log_score> forward_scores, backward_scores;
    std::vector<uint64_t> residue_offsets, region_offsets;
    std::vector<float> begin, end, occ;
    std::vector<msv_dom_region> regions;
};
struct Decoded_sequence {
    double forward_score = 0, backward_score = 0;
    std::vector<double> begin, end, occ;
};
// The split stage (msv.h "Split stage"): the items to align in place of the regions of an Envelopes.
// A region that is not multi-domain is its own item (prob 1); a multi-domain region is replaced by its clusters'
// envelopes (none if no cluster passes).  items[j] came from regions[region[j]].
struct Split_regions {
    std::vector<msv_aln_item> items;
    std::vector<uint64_t> region;
    std::vector<float> prob;
    std::vector<uint8_t> multidomain;  // per region
    uint64_t truncated = 0;            // samples that met a zero total weight
};
class Domain_HMM {
  public:
    explicit Domain_HMM(const Profile_HMM& base_hmm, int device = 0, msv_insert_mode inserts = MSV_INSERTS_ZERO);
    ~Domain_HMM();
    Domain_HMM(const Domain_HMM&) = delete;
    Domain_HMM& operator=(const Domain_HMM&) = delete;

    Decoded_sequence decode_on_sequence(const Protein_sequence& seq);
    // select empty = every sequence; workspace_bytes 0 = the default (1 GiB)
    Envelopes decode_batch(const Packed_sequences& packed, const std::vector<uint32_t>& select = {},
                           float rt1 = 0.25f, float rt2 = 0.10f, uint64_t workspace_bytes = 0);
    // HMMER3's treatment of multi-domain regions: msv_dom_is_multidomain(rt3) on every region of `envelopes` (made by
    // decode_batch on `packed`), msv_spl_sample_batch on the multi-domain ones, msv_spl_cluster with its defaults
    Split_regions split_regions(const Packed_sequences& packed, const Envelopes& envelopes, float rt3 = 0.20f,
                                uint32_t n_samples = 200, uint64_t seed = 42, uint64_t workspace_bytes = 0);

    msv_dom_profile* handle() { return profile_; }
    size_t model_length() const { return model_length_; }

  private:
    size_t model_length_ = 0;
    bool inserts_ = false;
    std::vector<float> match_scores_, insert_scores_, transition_scores_;  // [20][M], [20][M], [M][7]
    float tr_B_Mk_ = 0, tr_E_C_ = 0, tr_E_J_ = 0;
    msv_dom_profile* profile_ = nullptr;
};

// The bias filter (msv.h "Bias filter"): HMMER3's composition filter, the Forward score of a two-state
// HMM (background / the profile's COMPO composition) over each sequence, in nats.  Same surface as Forward_HMM:
// run_on_sequence is the float64 CPU definition (msv_bf_cpu_score), the reference of every test;
// parallel_run_on_sequence and score_batch the gfx950 kernel (float32, within msv.h's tolerance of it); pvalues are
// the filtered P-values of a stage's scores (msv_bf_pvalues).  Header-only: every method is one C-ABI call.
class Bias_filter {
  public:
    // compo: the profile's COMPO line (profile_compo(file_path)); the second form reads both from the file
    Bias_filter(const Profile_HMM& base_hmm, const Probabilities_array<NUM_OF_AMINO_ACIDS>& compo, int device = 0)
        : model_length_(base_hmm.model_length), compo_(compo) {
        const msv_status s = msv_bf_profile_create(device, compo_.data(), msv_background_frequencies(),
                                                   static_cast<uint32_t>(model_length_), &profile_);
        if (s != MSV_OK) throw msv_error(s, std::string("msv_bf_profile_create: ") + msv_status_string(s));
    }
    explicit Bias_filter(const std::string& file_path, int device = 0)
        : Bias_filter(Profile_HMM(file_path), profile_compo(file_path), device) {}
    ~Bias_filter() { msv_bf_profile_destroy(profile_); }
    Bias_filter(const Bias_filter&) = delete;
    Bias_filter& operator=(const Bias_filter&) = delete;

    double run_on_sequence(const Protein_sequence& seq) {
        const Packed_sequences p = Packed_sequences::pack({seq});
        double bias = 0;
        check(msv_bf_cpu_score(compo_.data(), msv_background_frequencies(), static_cast<uint32_t>(model_length_),
                               p.codes.data(), p.codes.size(), &bias),
              "msv_bf_cpu_score");
        return bias;
    }
    Log_score parallel_run_on_sequence(const Protein_sequence& seq) { return score_batch(Protein_sequences{seq})[0]; }
    std::vector<Log_score> score_batch(const Protein_sequences& seqs) {
        return score_batch(Packed_sequences::pack(seqs));
    }
    std::vector<Log_score> score_batch(const Packed_sequences& packed) {
        std::vector<Log_score> out(packed.size());
        check(msv_bf_score_batch(profile_, packed.codes.data(), packed.offsets.data(), packed.size(), out.data(),
                                 nullptr),
              "msv_bf_score_batch");
        return out;
    }
    // kind: MSV_BF_GUMBEL with (mu, lambda), MSV_BF_EXPONENTIAL with (tau, lambda)
    std::vector<double> pvalues(const std::vector<Log_score>& scores, const std::vector<Log_score>& bias,
                                const Packed_sequences& packed, float location, float scale, int kind) const {
        if (scores.size() != packed.size() || bias.size() != packed.size())
            throw msv_error(MSV_ERR_INVALID_ARGUMENT, "scores, bias and sequences disagree");
        std::vector<double> out(packed.size());
        check(msv_bf_pvalues(scores.data(), bias.data(), packed.offsets.data(), packed.size(), location, scale, kind,
                             out.data()),
              "msv_bf_pvalues");
        return out;
    }

    msv_bf_profile* handle() { return profile_; }
    size_t model_length() const { return model_length_; }
    const Probabilities_array<NUM_OF_AMINO_ACIDS>& compo() const { return compo_; }

  private:
    static void check(msv_status s, const char* what) {
        if (s == MSV_ERR_BAD_RESIDUE) throw std::out_of_range("residue outside the 20 amino acids");
        if (s != MSV_OK) throw msv_error(s, std::string(what) + ": " + msv_status_string(s));
    }
    size_t model_length_ = 0;
    Probabilities_array<NUM_OF_AMINO_ACIDS> compo_{};
    msv_bf_profile* profile_ = nullptr;
};

// Calibration (msv.h "Calibration"): HMMER3's p7_Calibrate for this library's engines, on the GPU.
// stats is msv_hmm_stats' six with the slots of every engine given replaced by the fitted values (a null engine keeps
// the file's); from_file the file's own six; report the float64 values.  Header-only: one C-ABI call.
struct Calibration {
    std::array<float, 6> stats{};
    std::array<float, 6> from_file{};
    msv_cal_report report{};
};
inline Calibration calibrate(const std::string& file_path, MSV_HMM* msv_engine, Viterbi_HMM* vit_engine,
                             Forward_HMM* fwd_engine, const msv_cal_options* options = nullptr) {
    msv_hmm* h = nullptr;
    msv_status s = msv_hmm_read(file_path.c_str(), &h);
    if (s != MSV_OK) throw msv_error(s, std::string(msv_status_string(s)) + ": " + file_path);
    Calibration c;
    msv_hmm_stats(h, c.from_file.data());
    c.stats = c.from_file;
    c.report.struct_size = sizeof(c.report);
    s = msv_cal_calibrate(h, msv_engine ? msv_engine->handle() : nullptr, vit_engine ? vit_engine->handle() : nullptr,
                          fwd_engine ? fwd_engine->handle() : nullptr, options, c.stats.data(), &c.report);
    msv_hmm_destroy(h);
    if (s != MSV_OK) throw msv_error(s, std::string("msv_cal_calibrate: ") + msv_status_string(s));
    return c;
}

// The emit stage (msv.h "Emit stage"): sequences drawn from a profile, this library's own scoring model
// run forwards, with the true path of each.  cpu_emit is the definition (msv_emit_generate); emit the gfx950 kernels
// (msv_emit_batch), byte for byte the same.  Header-only: every method is a few C-ABI calls.
struct Emitted {
    Packed_sequences sequences;
    std::vector<uint8_t> truncated;
    Viterbi_traces truth;  // domains and ops of every sequence; scores are left empty (msv_emit_path_score gives one)
    uint64_t chunks = 0;
};
class Emit_HMM {
  public:
    explicit Emit_HMM(const std::string& file_path, const msv_emit_options* options = nullptr, int device = 0) {
        msv_status s = msv_hmm_read(file_path.c_str(), &hmm_);
        if (s != MSV_OK) throw msv_error(s, std::string(msv_status_string(s)) + ": " + file_path);
        if (options) {
            options_ = *options;
            has_options_ = true;
        }
        s = msv_emit_profile_create(device, hmm_, has_options_ ? &options_ : nullptr, &profile_);
        if (s != MSV_OK) {
            msv_hmm_destroy(hmm_);
            throw msv_error(s, std::string("msv_emit_profile_create: ") + msv_status_string(s));
        }
    }
    ~Emit_HMM() {
        msv_emit_profile_destroy(profile_);
        msv_hmm_destroy(hmm_);
    }
    Emit_HMM(const Emit_HMM&) = delete;
    Emit_HMM& operator=(const Emit_HMM&) = delete;

    Emitted cpu_emit(uint64_t n, uint64_t seed = 42, uint64_t first = 0) const {
        msv_emit_result* r = nullptr;
        check(msv_emit_generate(hmm_, has_options_ ? &options_ : nullptr, seed, first, n, &r), "msv_emit_generate");
        return take(r);
    }
    // workspace_bytes 0 = the default (256 MiB); the bytes do not depend on it
    Emitted emit(uint64_t n, uint64_t seed = 42, uint64_t first = 0, bool truth = true, uint64_t workspace_bytes = 0) {
        msv_emit_result* r = nullptr;
        check(msv_emit_batch(profile_, seed, first, n, truth ? 1 : 0, workspace_bytes, nullptr, &r), "msv_emit_batch");
        return take(r);
    }
    msv_emit_info describe() const {
        msv_emit_info info{};
        info.struct_size = sizeof(info);
        check(msv_emit_describe(profile_, &info), "msv_emit_describe");
        return info;
    }
    msv_emit_profile* handle() { return profile_; }

  private:
    static void check(msv_status s, const char* what) {
        if (s != MSV_OK) throw msv_error(s, std::string(what) + ": " + msv_status_string(s));
    }
    static Emitted take(msv_emit_result* r) {
        Emitted e;
        e.sequences.codes.resize(msv_emit_result_residues(r));
        e.sequences.offsets.resize(msv_emit_result_count(r) + 1);
        e.truncated.resize(msv_emit_result_count(r));
        e.truth.domain_offsets.resize(msv_emit_result_count(r) + 1);
        e.truth.domains.resize(msv_emit_result_domains(r));
        e.truth.ops.resize(msv_emit_result_ops(r));
        e.chunks = msv_emit_result_chunks(r);
        const msv_status s =
            msv_emit_result_copy(r, e.sequences.codes.data(), e.sequences.offsets.data(), e.truth.domain_offsets.data(),
                                 e.truth.domains.data(), e.truth.ops.data(), e.truncated.data());
        msv_emit_result_free(r);
        check(s, "msv_emit_result_copy");
        return e;
    }
    msv_hmm* hmm_ = nullptr;
    msv_emit_options options_{};
    bool has_options_ = false;
    msv_emit_profile* profile_ = nullptr;
};
