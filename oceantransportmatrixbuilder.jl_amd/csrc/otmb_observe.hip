// otmb_observe.hip -- observations of a state, obs[j, c] = Σ_i W[i, j]·X[i, c] for q observers (the columns of W) and k tracers, and in the
// same pass the time-weighted mean Xbar += tw·X: otmb_op_observe[_dev], and the pass otmb_op_step_obs[_dev] runs after every completed step
// (otmb_step.hip; ob_pass below).  include/otmb.h states the order as a contract; tests/observe_ref.py restates it in numpy.
//
// The order is the periodic layer's for Vᵀ·w (otmb_periodic.hip): a workgroup of 256 lanes takes OB_ROWS = 2048 rows, lane t the row pairs
// t, t + 256, t + 512, t + 768 of them in that order; one accumulator per (observer, tracer) from +0.0, product and sum separate operations
// (no FMA: -ffp-contract=off); the workgroup's tree is otmb_op_sum.h's; ONE partial per workgroup and entry; ob_fold_kernel adds an entry's
// partials in workgroup order from partial 0.  An entry's accumulator, tree and fold are its own, so entry (j, c) has the bits that observer
// and that tracer have alone: a register block (QB observers x KB tracers, each 4 / 2 / 1 by op_blocks) shares loads, never arithmetic.
// X is read once per pair of blocks and W likewise; the mean is updated by the first observer block of a tracer block, from the X values
// that block loaded anyway.  The pair loads and the row dealing are copies of otmb_periodic.hip's pd_load / pd_store / pd_row, which the host
// tests of that file compile from its text as it stands.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "otmb_op_sum.h"
#include "otmb_solve.h"

#define OB_ROWS 2048  // rows per workgroup: 256 lanes x 4 pairs
#define OB_NB 4       // the largest register block of observers and of tracers (op_blocks: 4, 2, 1)

struct Ob2 {
    double a, b;
};
// rows i (even) and i + 1 of p; row i + 1 counts only below n.  al: p + i is 16-byte aligned (p is, and its leading dimension is even).
__device__ __forceinline__ Ob2 ob_load(const double *__restrict__ p, i64 i, i64 n, bool al) {
    if (al && i + 1 < n) {
        const double2 v = *reinterpret_cast<const double2 *>(p + i);
        return {v.x, v.y};
    }
    return {p[i], i + 1 < n ? p[i + 1] : 0.0};
}
__device__ __forceinline__ void ob_store(double *__restrict__ p, i64 i, i64 n, bool al, Ob2 v) {
    if (al && i + 1 < n) {
        *reinterpret_cast<double2 *>(p + i) = make_double2(v.a, v.b);
        return;
    }
    p[i] = v.a;
    if (i + 1 < n) p[i + 1] = v.b;
}
// the p-th row pair of this lane: its first row (>= n: the lane is done)
__device__ __forceinline__ i64 ob_row(int p) { return 2 * ((i64)blockIdx.x * (OB_ROWS / 2) + threadIdx.x + 256 * p); }

struct ObMean {  // the mean's update: Xbar = (first ? +0.0 : Xbar) + tw·X
    double *xbar;
    i64 ldm;
    double tw;
    bool al, first;
};

// QB observers (0: none, the pass only updates the mean) x KB tracers; MEAN: this launch updates the mean of its tracers.
// part: the partials of the block's first entry; entry (j, c) of the block at part[(j + q·c)·np + workgroup].
template <int QB, int KB, bool MEAN>
__global__ __launch_bounds__(256) void ob_kernel(i64 n, const double *__restrict__ W, i64 ldw, bool alw, const double *__restrict__ X, i64 ldx, bool alx,
                                                 double *__restrict__ part, i64 np, i64 q, ObMean m) {
    constexpr int NV = QB * KB > 0 ? QB * KB : 1;
    double acc[NV];
#pragma unroll
    for (int e = 0; e < NV; ++e) acc[e] = 0.0;
    for (int p = 0; p < OB_ROWS / 512; ++p) {
        const i64 i = ob_row(p);
        if (i >= n) break;
        Ob2 x[KB];
#pragma unroll
        for (int c = 0; c < KB; ++c) x[c] = ob_load(X + c * ldx, i, n, alx);
        if constexpr (MEAN) {
#pragma unroll
            for (int c = 0; c < KB; ++c) {
                Ob2 s = {0.0, 0.0};
                if (!m.first) s = ob_load(m.xbar + c * m.ldm, i, n, m.al);
                const double pa = m.tw * x[c].a;
                s.a = s.a + pa;
                const double pb = m.tw * x[c].b;
                s.b = s.b + pb;
                ob_store(m.xbar + c * m.ldm, i, n, m.al, s);
            }
        }
#pragma unroll
        for (int j = 0; j < QB; ++j) {
            const Ob2 w = ob_load(W + j * ldw, i, n, alw);
#pragma unroll
            for (int c = 0; c < KB; ++c) {
                const double pa = w.a * x[c].a;
                acc[j * KB + c] = acc[j * KB + c] + pa;
                if (i + 1 < n) {
                    const double pb = w.b * x[c].b;
                    acc[j * KB + c] = acc[j * KB + c] + pb;
                }
            }
        }
    }
    if constexpr (QB > 0) {
        __shared__ double red[4 * NV];
        op_block_sum<NV>(acc, red);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int j = 0; j < QB; ++j)
#pragma unroll
                for (int c = 0; c < KB; ++c) part[((i64)j + q * c) * np + blockIdx.x] = acc[j * KB + c];
        }
    }
}

// lane l's v in every lane (l is wave-uniform): two v_readlane_b32 into scalar registers, no LDS round trip
__device__ __forceinline__ double ob_lane_value(double v, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}
// one wave per entry: out[e] = the entry's np partials added in workgroup order from partial 0 (np == 0: +0.0).  The chain of np dependent
// additions is the contract, so the rest is kept off it: the wave loads OB_FOLD x 64 partials at once (OB_FOLD loads in flight per lane),
// then every lane adds them in order out of the lanes' registers.
#define OB_FOLD 8
__global__ __launch_bounds__(64) void ob_fold_kernel(const double *__restrict__ part, i64 np, double *__restrict__ out) {
    const double *p = part + (i64)blockIdx.x * np;
    double s = 0.0;
    for (i64 b0 = 0; b0 < np; b0 += 64 * OB_FOLD) {
        double v[OB_FOLD];
#pragma unroll
        for (int u = 0; u < OB_FOLD; ++u) {
            const i64 b = b0 + 64 * u + threadIdx.x;
            v[u] = b < np ? p[b] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < OB_FOLD; ++u) {
            const i64 c0 = b0 + 64 * u;
            const int m = np - c0 >= 64 ? 64 : np - c0 > 0 ? (int)(np - c0) : 0;
            if (m == 64) {
#pragma unroll
                for (int l = 0; l < 64; ++l) {
                    const double w = ob_lane_value(v[u], l);
                    s = c0 + l == 0 ? w : s + w;
                }
            } else {
                for (int l = 0; l < m; ++l) {
                    const double w = ob_lane_value(v[u], l);
                    s = c0 + l == 0 ? w : s + w;
                }
            }
        }
    }
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
static bool ob_aligned(const void *p, i64 ld) { return ((uintptr_t)p & 15) == 0 && (ld & 1) == 0; }

int32_t ob_reserve(otmb_op *op, i64 k, i64 q) {
    const i64 np = (op->n + OB_ROWS - 1) / OB_ROWS;
    return otmb_reserve(op->ctx, op->ob, std::max<size_t>((size_t)(q * k * np) * 8, 8));
}

void ob_pass(otmb_op *op, i64 k, i64 q, const double *W, i64 ldw, const double *X, i64 ldx, double *obs, double *Xbar, i64 ldm, double tw, bool first) {
    hipStream_t st = op->ctx->stream;
    const i64 n = op->n, np = (n + OB_ROWS - 1) / OB_ROWS;
    double *part = (double *)op->ob.p;
    if (np > 0 && (q > 0 || Xbar)) {
        const bool alw = ob_aligned(W, ldw), alx = ob_aligned(X, ldx);
        const dim3 grid((unsigned)np), block(256);
        op_blocks<OB_NB>(0, k, [&](auto kb, i64 c0) {
            constexpr int KB = decltype(kb)::value;
            const ObMean m = {Xbar ? Xbar + c0 * ldm : nullptr, ldm, tw, ob_aligned(Xbar, ldm), first};
            const double *Xc = X + c0 * ldx;
            if (q == 0) {
                hipLaunchKernelGGL((ob_kernel<0, KB, true>), grid, block, 0, st, n, W, ldw, alw, Xc, ldx, alx, part, np, q, m);
                return;
            }
            op_blocks<OB_NB>(0, q, [&](auto qb, i64 j0) {
                constexpr int QB = decltype(qb)::value;
                double *pc = part + (j0 + q * c0) * np;
                if (Xbar && j0 == 0)
                    hipLaunchKernelGGL((ob_kernel<QB, KB, true>), grid, block, 0, st, n, W + j0 * ldw, ldw, alw, Xc, ldx, alx, pc, np, q, m);
                else
                    hipLaunchKernelGGL((ob_kernel<QB, KB, false>), grid, block, 0, st, n, W + j0 * ldw, ldw, alw, Xc, ldx, alx, pc, np, q, m);
            });
        });
    }
    if (q > 0) hipLaunchKernelGGL(ob_fold_kernel, dim3((unsigned)(q * k)), dim3(64), 0, st, (const double *)part, np, obs);
}

const char *ob_complaint(const otmb_op *op, bool step, i64 nsteps, i64 q, const double *W, i64 ldw, const double *obs, const double *tw, const double *Xbar,
                         i64 ldm) {
#define OB_SAY(text) (step ? "otmb_op_step_obs: " text : "otmb_op_observe: " text)
    if (q < 0 || q >= (1ll << 31)) return OB_SAY("q (observers) must be >= 0");
    if (q > 0 && (!W || !obs)) return OB_SAY("W and obs must not be null when q > 0");
    if (q > 0 && ldw < op->n) return OB_SAY("ldw is smaller than the rows of W");
    if ((tw == nullptr) != (Xbar == nullptr)) return OB_SAY("tw and Xbar are given together or not at all");
    if (tw) {
        for (i64 t = 0; t < nsteps; ++t)
            if (!std::isfinite(tw[t])) return OB_SAY("a time weight is not finite");
        if (ldm < op->n) return OB_SAY("ldm is smaller than the rows of Xbar");
    }
#undef OB_SAY
    return nullptr;
}

static int32_t ob_check(otmb_op *op, int64_t k, int64_t q, const double *W, int64_t ldw, const double *X, int64_t ldx, const double *obs) {
    const auto fail = [&](const char *m) { return otmb_fail(op->ctx, OTMB_ERR_INVALID_ARG, m); };
    if (k < 1 || k >= (1ll << 31)) return fail("otmb_op_observe: k (tracers) must be >= 1");
    if (ldx < op->n) return fail("otmb_op_observe: ldx is smaller than the rows of X");
    if (op->n > 0 && !X) return fail("otmb_op_observe: null argument");
    const char *more = ob_complaint(op, false, 0, q, W, ldw, obs, nullptr, nullptr, 0);
    return more ? fail(more) : OTMB_OK;
}

extern "C" {

int32_t otmb_op_observe_dev(otmb_op *op, int64_t k, int64_t q, const double *W, int64_t ldw, const double *X, int64_t ldx, double *obs) {
    if (!op) return OTMB_ERR_INVALID_ARG;
    int32_t rc;
    if ((rc = ob_check(op, k, q, W, ldw, X, ldx, obs))) return rc;
    if (q == 0) return OTMB_OK;
    otmb_ctx *ctx = op->ctx;
    HIP_TRY(ctx, hipSetDevice(op->device));
    if ((rc = ob_reserve(op, k, q))) return rc;
    ob_pass(op, k, q, W, ldw, X, ldx, obs, nullptr, 0, 0.0, false);
    HIP_TRY(ctx, hipGetLastError());
    return OTMB_OK;
}

int32_t otmb_op_observe(otmb_op *op, int64_t k, int64_t q, const double *W, int64_t ldw, const double *X, int64_t ldx, double *obs) {
    if (!op) return OTMB_ERR_INVALID_ARG;
    int32_t rc;
    if ((rc = ob_check(op, k, q, W, ldw, X, ldx, obs))) return rc;
    if (q == 0) return OTMB_OK;
    otmb_ctx *ctx = op->ctx;
    const i64 n = op->n;
    HIP_TRY(ctx, hipSetDevice(op->device));
    // op->oh: obs (q x k) | W (n x q) | X (n x k), the matrices staged compactly
    if ((rc = otmb_reserve(ctx, op->oh, (size_t)(q * k + n * q + n * k) * 8))) return rc;
    double *dobs = (double *)op->oh.p, *dw = dobs + q * k, *dx = dw + n * q;
    if (n > 0 && ((rc = op_upload(ctx, dw, W, ldw, n, q)) || (rc = op_upload(ctx, dx, X, ldx, n, k)))) return rc;
    if ((rc = otmb_op_observe_dev(op, k, q, dw, n, dx, n, dobs))) return rc;
    return op_finish(ctx, OTMB_OK, obs, q * k, dobs, q * k, 1);
}

}  // extern "C"
