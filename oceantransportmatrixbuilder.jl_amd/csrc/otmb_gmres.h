// otmb_gmres.h -- the least-squares problem of one GMRES(m) column, on the host in double: the Hessenberg column the device's two
// Gram-Schmidt passes leave becomes a column of the triangle R by the old Givens rotations and a new one, the rotated right-hand side gives
// the recursive residual, and the triangle gives y at a restart.  otmb_periodic.hip holds one record per column; tests/periodic_ref.py
// (givens_column) restates push, and tests/test_gmres_host.py compares the two bit for bit.  Plain C++17: nothing of HIP, nothing of the
// library, so a host compiler takes this header alone.  One operation per statement where the order is the contract (build without FMA).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

struct GmresLsq {
    int64_t m = 0, i = 0;               // the restart length; the columns pushed since start
    std::vector<double> R, cs, sn, gv;  // the triangle (column i at R[i * (m + 1) ..]), the rotations, the rotated right-hand side

    // a new Krylov space from a residual of norm beta: the rotated right-hand side is β·e_0
    void start(int64_t m_, double beta) {
        m = m_, i = 0;
        R.assign((size_t)((m + 1) * m), 0.0), cs.assign((size_t)m, 0.0), sn.assign((size_t)m, 0.0), gv.assign((size_t)(m + 1), 0.0);
        gv[0] = beta;
    }

    // Column i from the two passes' h1 and h2 (i + 2 entries each, as the device leaves them; ‖w‖² in h2[i + 1]): H(0..i, i) = h1 + h2,
    // hn = H(i + 1, i) = ‖w‖, est = the recursive residual |γ_{i+1}|.  false: an input is not finite -- only R's column i has been
    // written, i stands, and the caller stops the column.
    bool push(const double *h1, const double *h2, double *hn, double *est) {
        double *r = R.data() + i * (m + 1);
        bool finite = std::isfinite(h1[i + 1]) && std::isfinite(h2[i + 1]);
        for (int64_t j = 0; j <= i; ++j) {
            r[j] = h1[j] + h2[j];
            finite = finite && std::isfinite(r[j]);
        }
        *hn = std::sqrt(h2[i + 1]);
        if (!finite) return false;
        for (int64_t j = 0; j < i; ++j) {  // the old rotations, then the one that clears H(i + 1, i)
            const double t = cs[(size_t)j] * r[j] + sn[(size_t)j] * r[j + 1];
            r[j + 1] = cs[(size_t)j] * r[j + 1] - sn[(size_t)j] * r[j];
            r[j] = t;
        }
        const double rr = std::hypot(r[i], *hn);
        cs[(size_t)i] = rr > 0.0 ? r[i] / rr : 1.0;
        sn[(size_t)i] = rr > 0.0 ? *hn / rr : 0.0;
        r[i] = rr;
        gv[(size_t)(i + 1)] = -(sn[(size_t)i] * gv[(size_t)i]);
        gv[(size_t)i] = cs[(size_t)i] * gv[(size_t)i];
        i += 1;
        *est = std::fabs(gv[(size_t)i]);
        return true;
    }

    // y (i entries) from the triangle: back substitution, term by term
    void solve(double *y) const {
        for (int64_t a = i - 1; a >= 0; --a) {
            double s = gv[(size_t)a];
            for (int64_t b = a + 1; b < i; ++b) {
                const double t = R[(size_t)(b * (m + 1) + a)] * y[b];
                s = s - t;
            }
            y[a] = s / R[(size_t)(a * (m + 1) + a)];
        }
    }
};
