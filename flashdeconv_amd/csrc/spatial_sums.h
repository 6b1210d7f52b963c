// Layout of the packed device result of the spatial-sums entries (fdx_spatial_autocorr_dev, fdx_spatial_perm_dev,
// fdx_local_stats_dev): one block of doubles the kernels write, one download, one unpack.  Plain host code (no HIP): the offsets are
// tested by hosttest/plan_asan.cpp.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "perm_plan.h"

namespace fdx {

// Offsets in doubles from the start of the block, for K columns (KK = K * K):
//   observed     [mean K | m2 K | C KK | sum deg, sum deg^2 as int64]                                        observed_doubles
//   permutation  the observed block, then [m4 K | the base's count_ge, count_le, sum_d, sumsq_d of KK each]        perm_doubles
struct SpatialSumsLayout : NullSumsLayout {
    size_t K, KK;
    size_t mean = 0, m2 = 0, C = 0, deg_sums = 0, observed_doubles = 0, m4 = 0, perm_doubles = 0;
    explicit SpatialSumsLayout(int k = 0) : K((size_t)k), KK((size_t)k * k) {
        m2 = mean + K;
        C = m2 + K;
        deg_sums = C + KK;
        observed_doubles = deg_sums + 2;
        m4 = observed_doubles;
        NullSumsLayout::operator=(NullSumsLayout(KK, m4 + K));
        perm_doubles = end;
    }
    // A downloaded block into the caller's arrays.  deg_sums_out: two int64.  C_out null: not wanted.  m4_out null: an observed
    // block, the five permutation arrays are not touched.
    void unpack(const double* h, double* mean_out, double* m2_out, double* C_out, int64_t* deg_sums_out, double* m4_out = nullptr,
                int64_t* count_ge_out = nullptr, int64_t* count_le_out = nullptr, double* sum_d_out = nullptr,
                double* sumsq_d_out = nullptr) const {
        std::copy(h + mean, h + mean + K, mean_out);
        std::copy(h + m2, h + m2 + K, m2_out);
        if (C_out) std::copy(h + C, h + C + KK, C_out);
        std::memcpy(deg_sums_out, h + deg_sums, 2 * sizeof(int64_t));
        if (!m4_out) return;
        std::copy(h + m4, h + m4 + K, m4_out);
        NullSumsLayout::unpack(h, count_ge_out, count_le_out, sum_d_out, sumsq_d_out);
    }
    // The answers without spots: no mean, zero sums (C_out, m4_out may be null).
    void fill_empty(double* mean_out, double* m2_out, double* C_out, double* m4_out = nullptr) const {
        std::fill(mean_out, mean_out + K, std::nan(""));
        std::fill(m2_out, m2_out + K, 0.0);
        if (C_out) std::fill(C_out, C_out + KK, 0.0);
        if (m4_out) std::fill(m4_out, m4_out + K, 0.0);
    }
};

}  // namespace fdx
