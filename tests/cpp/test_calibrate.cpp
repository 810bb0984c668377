// test_calibrate.cpp -- the C++ calibrate() (msv_hmm.hpp) on a profile given by the caller: the default calibration
// with the three engines, then one with the Viterbi engine alone.  The slots of a null engine must keep the file's
// values, every lambda slot written must be the profile's, and a second run must return the same bits.  The six floats
// are printed as hexadecimal bit patterns for the caller to compare (tests/test_gpu_calibrate.py compares them with
// the Python surface's).
// Usage: test_calibrate <profile.hmm>   (exit 0 = pass)
#include <cstdio>
#include <cstring>
#include <string>

#include "msv_hmm.hpp"

#define REQUIRE(cond)                                                                \
    do {                                                                             \
        if (!(cond)) {                                                               \
            std::printf("test_calibrate failed! %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                                \
        }                                                                            \
    } while (0)

int main(int argc, char** argv) {
    if (argc < 2) {
        std::printf("usage: test_calibrate <profile.hmm>\n");
        return 2;
    }
    const std::string path = argv[1];
    const Profile_HMM prof(path);
    MSV_HMM msv(prof);
    Viterbi_HMM vit(prof);
    Forward_HMM fwd(prof);
    const Calibration all = calibrate(path, &msv, &vit, &fwd);
    REQUIRE(all.report.ran == 7 && all.report.seed == 42 && all.report.tail == 0.04);
    REQUIRE(all.from_file[0] == prof.stats_local_msv_mu && all.from_file[4] == prof.stats_local_forward_theta);
    for (int s = 0; s < 3; ++s) {
        REQUIRE(all.stats[2 * s] == static_cast<float>(all.report.location[s]));
        REQUIRE(all.stats[2 * s + 1] == static_cast<float>(all.report.lambda));
        REQUIRE(all.report.chunks[s] == 1);
    }
    const Calibration again = calibrate(path, &msv, &vit, &fwd);
    REQUIRE(std::memcmp(all.stats.data(), again.stats.data(), sizeof(float) * 6) == 0);
    const Calibration only = calibrate(path, nullptr, &vit, nullptr);
    REQUIRE(only.report.ran == 2 && only.stats[2] == all.stats[2] && only.stats[3] == all.stats[3]);
    REQUIRE(only.stats[0] == prof.stats_local_msv_mu && only.stats[1] == prof.stats_local_msv_lambda);
    REQUIRE(only.stats[4] == prof.stats_local_forward_theta && only.stats[5] == prof.stats_local_forward_lambda);
    msv_cal_options o{};
    o.struct_size = sizeof(o);
    o.n[0] = 1;
    bool refused = false;
    try {
        (void)calibrate(path, &msv, nullptr, nullptr, &o);
    } catch (const msv_error& e) {
        refused = e.status == MSV_ERR_INVALID_ARGUMENT;
    }
    REQUIRE(refused);
    std::printf("stats");
    for (float v : all.stats) {
        uint32_t u;
        std::memcpy(&u, &v, sizeof(u));
        std::printf(" %08x", u);
    }
    std::printf("\ntest_calibrate passed\n");
    return 0;
}
