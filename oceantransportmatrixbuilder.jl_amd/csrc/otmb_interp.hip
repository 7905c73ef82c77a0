// otmb_interp.hip -- (1 - w)·(slot a) + w·(slot b) into the operator's private value set op->interp: the matrix of a blended step of
// otmb_op_step_interp[_dev] (otmb_step.hip) and, through it, of otmb_op_periodic_interp[_dev].  include/otmb.h states the contract;
// tests/interp_ref.py restates it.
//
// Per stored entry: pa = wa * va, pb = wb * vb, v = pa + pb, one operation per statement, no FMA (-ffp-contract=off): the fold of
// otmb_op_combine_slots for two terms (IEEE addition commutes, so which of the two slots comes first cannot matter).  wa = 1.0 - w is the
// host's one subtraction; both weights travel as kernel arguments.
//
// ONE launch writes both value arrays of op->interp -- nzval of the CSC copy (nnz entries) and the row layout's values (nval entries, padding
// included: never read by a product, so what the arithmetic makes of it does not matter).  The two arrays are separate allocations, so
// the work is cut into chunks of IP_SPAN entries PER ARRAY, the chunks of nzval first, and a chunk is indexed from its own array's base:
// every base is an allocation's, hence 16-byte aligned, whatever the parity of nnz (one range over both would put the second array on an
// odd entry after an odd nnz).  In a chunk lane t takes the entry pairs t, t + 256, t + 512, t + 768 as 16-byte loads and stores; the last
// entry of an odd count goes alone.  The four pairs' loads of both sources are issued before the first is used (eight loads in flight a lane).
//
// Bytes: 24 per entry of nnz + nval (two reads, one write), nothing else: no table, no loop over terms, no host synchronisation.
// Grid: at most IP_GRID workgroups of 256 lanes, each striding over the chunks.  IP_GRID = 1792 is 7 workgroups per CU on the 256 CUs, one
// wave of each per SIMD: the kernel needs 50 VGPRs, no LDS and no scratch, but its 82 SGPRs (two arrays' pointers and counts as
// arguments) admit 7 workgroups of 256 lanes per CU where 80 would admit 8, so 7 waves per SIMD is what is resident, and the cap is set
// to that, not to the 8 the occupancy figure of the compiler prints.  At the 1 degree size (20.7 M + 21.3 M entries, 20 512 chunks) the cap
// binds and the kernel runs at those 7 waves per SIMD.  A streaming kernel has nothing but loads in flight to hide HBM's latency with,
// so it wants every wave slot it can have; more workgroups than are resident would only queue behind them, so the rest of the chunks are
// strided over instead.  The grid is then shrunk until every workgroup takes the same number of chunks (20 512 chunks: 1710 workgroups
// of 12, not 1792 of 11 or 12): with all of them resident from the start, a workgroup with one chunk more than the others would be a
// tail of a twelfth of the run at a fraction of the bandwidth.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "otmb_solve.h"

#define IP_SPAN 2048  // entries per chunk: 256 lanes x 4 pairs
#define IP_GRID 1792  // the most workgroups of a launch: 7 per CU, what 82 SGPRs admit

struct Ip2 {
    double a, b;
};
// entries i (even) and i + 1 of p; entry i + 1 counts only below count
__device__ __forceinline__ Ip2 ip_load(const double *__restrict__ p, i64 i, i64 count) {
    if (i + 1 < count) {
        const double2 v = *reinterpret_cast<const double2 *>(p + i);
        return {v.x, v.y};
    }
    return {p[i], 0.0};
}
__device__ __forceinline__ void ip_store(double *__restrict__ p, i64 i, i64 count, Ip2 v) {
    if (i + 1 < count) {
        *reinterpret_cast<double2 *>(p + i) = make_double2(v.a, v.b);
        return;
    }
    p[i] = v.a;
}

struct IpArray {  // one value array: the two sources, the destination and its entries
    const double *a, *b;
    double *to;
    i64 count;
};

// chunks 0 .. cnz - 1 are nz's, cnz .. cnz + cval - 1 val's; the destination is neither source (op->interp is no slot)
__global__ __launch_bounds__(256) void ip_blend_kernel(IpArray nz, IpArray val, i64 cnz, i64 cval, double wa, double wb) {
    for (i64 ch = blockIdx.x; ch < cnz + cval; ch += gridDim.x) {
        const bool first = ch < cnz;  // (uniform over the workgroup)
        const double *__restrict__ sa = first ? nz.a : val.a, *__restrict__ sb = first ? nz.b : val.b;
        double *__restrict__ to = first ? nz.to : val.to;
        const i64 count = first ? nz.count : val.count, base = (first ? ch : ch - cnz) * IP_SPAN;
        Ip2 va[IP_SPAN / 512], vb[IP_SPAN / 512];
#pragma unroll
        for (int r = 0; r < IP_SPAN / 512; ++r) {
            const i64 i = base + 2 * (threadIdx.x + 256 * r);
            if (i < count) va[r] = ip_load(sa, i, count), vb[r] = ip_load(sb, i, count);
        }
#pragma unroll
        for (int r = 0; r < IP_SPAN / 512; ++r) {
            const i64 i = base + 2 * (threadIdx.x + 256 * r);
            if (i >= count) break;
            Ip2 v;
            const double pa0 = wa * va[r].a;
            const double pb0 = wb * vb[r].a;
            v.a = pa0 + pb0;
            const double pa1 = wa * va[r].b;
            const double pb1 = wb * vb[r].b;
            v.b = pa1 + pb1;
            ip_store(to, i, count, v);
        }
    }
}

// op->interp at the slots' exact sizes (allocated on first use, kept with the operator); may wait for the device: before a loop, never inside
int32_t ip_reserve(otmb_op *op) {
    for (DevBuf *b : {&op->interp.nz, &op->interp.val}) {
        const size_t bytes = std::max<size_t>((size_t)(b == &op->interp.nz ? op->nnz : op->nval) * 8, 8);
        if (b->p && b->cap == bytes) continue;
        if (b->p) (void)hipFree(b->p);
        b->p = nullptr, b->cap = 0;
        if (hipMalloc(&b->p, bytes) != hipSuccess) {
            (void)hipGetLastError();
            b->p = nullptr;
            return otmb_fail(op->ctx, OTMB_ERR_ALLOC, "hipMalloc (step_interp: the blended values)");
        }
        b->cap = bytes;
    }
    return OTMB_OK;
}

// wa·(slot a) + wb·(slot b) -> op->interp (reserved), both value arrays, enqueued on the context's stream
int32_t ip_blend(otmb_op *op, i64 a, i64 b, double wa, double wb) {
    otmb_ctx *ctx = op->ctx;
    const OpSlot &sa = op->slots[(size_t)a], &sb = op->slots[(size_t)b];
    const IpArray nz = {(const double *)sa.nz.p, (const double *)sb.nz.p, (double *)op->interp.nz.p, op->nnz};
    const IpArray val = {(const double *)sa.val.p, (const double *)sb.val.p, (double *)op->interp.val.p, op->nval};
    const i64 cnz = (op->nnz + IP_SPAN - 1) / IP_SPAN, cval = (op->nval + IP_SPAN - 1) / IP_SPAN;
    const i64 chunks = cnz + cval;
    if (chunks == 0) return OTMB_OK;
    const i64 each = (chunks + IP_GRID - 1) / IP_GRID, grid = (chunks + each - 1) / each;  // every workgroup takes `each` chunks (the last few one less): no tail
    hipLaunchKernelGGL(ip_blend_kernel, dim3((unsigned)grid), dim3(256), 0, ctx->stream, nz, val, cnz, cval, wa, wb);
    HIP_TRY(ctx, hipGetLastError());
    return OTMB_OK;
}
