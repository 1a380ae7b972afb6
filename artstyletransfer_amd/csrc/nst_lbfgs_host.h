// nst_lbfgs_host.h - the host scalars of the L-BFGS driver (nothing of HIP is needed here: tests/lbfgs_host.cpp drives this
// header alone): the line search's cubic interpolation, and the inner-product form of the two-loop recursion - the tables
// SY[i][j] = s_i . y_j and YY[i][j] = y_i . y_j over the curvature pairs held, how a multi-dot result fills them, and the
// coefficients of the direction.  nst_opt.cpp is the only user: its driver keeps one PairTables per optimiser, one
// multi-dot pass per step; nst_lbfgs_direction fills one with a pass per pair.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

namespace nst {

// torch:optim/lbfgs.py:12-37 on host scalars
inline double cubic_interpolate(double x1, double f1, double g1, double x2, double f2, double g2, bool has_bounds, double lo,
                                double hi) {
    double xmin = has_bounds ? lo : std::min(x1, x2);
    double xmax = has_bounds ? hi : std::max(x1, x2);
    const double d1 = g1 + g2 - 3 * (f1 - f2) / (x1 - x2);
    const double d2sq = d1 * d1 - g1 * g2;
    if (d2sq >= 0) {
        const double d2 = std::sqrt(d2sq);
        double min_pos;
        if (x1 <= x2) min_pos = x2 - (x2 - x1) * ((g2 + d2 - d1) / (g2 - g1 + 2 * d2));
        else min_pos = x1 - (x1 - x2) * ((g1 + d2 - d1) / (g1 - g2 + 2 * d2));
        return std::min(std::max(min_pos, xmin), xmax);
    }
    return (xmin + xmax) / 2.0;
}

// d = -H g by the two-loop recursion (lbfgs.py:444-460) carried out on inner products: with q0 = -g,
//   al_i = ro_i (s_i.q0 - sum_{j>i} al_j s_i.y_j)                                   (first loop, i = m-1 .. 0)
//   be_i = ro_i (H (y_i.q0 - sum_j al_j y_j.y_i) + sum_{j<i} (al_j - be_j) s_j.y_i)  (second loop, i = 0 .. m-1)
//   d = H q0 - H sum_j al_j y_j + sum_j (al_j - be_j) s_j
// The two recurrences on host scalars (SYm, YYm: row-major with leading dimension ld): coef[j] multiplies y_j, coef[m + j]
// multiplies s_j
inline void direction_coefficients(int m, int ld, const double* SYm, const double* YYm, const float* ro, float Hd,
                                   const double* sq, const double* yq, float* coef) {
    std::vector<double> al(m), be(m);
    for (int i = m - 1; i >= 0; --i) {
        double v = sq[i];                                             // s_i . q0
        for (int j = i + 1; j < m; ++j) v -= al[j] * SYm[(size_t)i * ld + j];
        al[i] = (double)ro[i] * v;
    }
    for (int i = 0; i < m; ++i) {
        double t = yq[i];                                             // y_i . q0
        for (int j = 0; j < m; ++j) t -= al[j] * YYm[(size_t)j * ld + i];
        double v = (double)Hd * t;
        for (int j = 0; j < i; ++j) v += (al[j] - be[j]) * SYm[(size_t)j * ld + i];
        be[i] = (double)ro[i] * v;
    }
    for (int j = 0; j < m; ++j) { coef[j] = (float)(-(double)Hd * al[j]); coef[m + j] = (float)(al[j] - be[j]); }
}

// SY and YY of up to `cap` pairs, oldest first.  A multi-dot result `res` over the 2m vectors y_0..y_{m-1}, s_0..s_{m-1}
// with the operands (a, b, c) holds three floats per vector v: a . v, b . v, c . v.
struct PairTables {
    int cap = 0;
    std::vector<double> SY, YY;          // cap x cap, row-major

    void reset(int capacity) {
        cap = capacity;
        SY.assign((size_t)cap * cap, 0.0);
        YY.assign((size_t)cap * cap, 0.0);
    }
    // the oldest pair leaves: rows / columns move up-left
    void evict_oldest() {
        for (int i = 0; i + 1 < cap; ++i)
            for (int j = 0; j + 1 < cap; ++j) {
                SY[(size_t)i * cap + j] = SY[(size_t)(i + 1) * cap + j + 1];
                YY[(size_t)i * cap + j] = YY[(size_t)(i + 1) * cap + j + 1];
            }
    }
    // row and column k of both tables from the result of a pass with a = s_k, b = y_k over m pairs
    void put_pair(int k, int m, const float* res) {
        for (int j = 0; j < m; ++j) {
            SY[(size_t)k * cap + j] = res[(size_t)j * 3 + 0];                                     // s_k . y_j
            YY[(size_t)k * cap + j] = YY[(size_t)j * cap + k] = res[(size_t)j * 3 + 1];           // y_k . y_j
            SY[(size_t)j * cap + k] = res[(size_t)(m + j) * 3 + 1];                               // s_j . y_k
        }
    }
    // the direction's coefficients from the result of a pass with c = q0 (any a, b) over m pairs
    void coefficients(int m, const float* res, const float* ro, float Hd, float* coef) const {
        std::vector<double> sq(m), yq(m);
        for (int i = 0; i < m; ++i) { sq[i] = res[(size_t)(m + i) * 3 + 2]; yq[i] = res[(size_t)i * 3 + 2]; }
        direction_coefficients(m, cap, SY.data(), YY.data(), ro, Hd, sq.data(), yq.data(), coef);
    }
};

}  // namespace nst
