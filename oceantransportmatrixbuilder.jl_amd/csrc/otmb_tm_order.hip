// otmb_tm_order.hip -- the order in which the fill pass (otmb_transportmatrix.hip) takes its tiles.
#include "otmb_tm.h"

#ifndef OTMB_MARCH_AUTO_ROWS
#define OTMB_MARCH_AUTO_ROWS 8  // tile order when the caller does not choose: march order, bands of 8 rows (with the matrices written by
                                // non-temporal stores: -8 % against wet-rank order at 1 and at 0.25 degree, R = 2 ... 32 within 1 %)
#endif
#ifndef OTMB_MARCH_AUTO_COLS
#define OTMB_MARCH_AUTO_COLS 1536  // ... and, on grids with longer rows, blocks of at most this many columns (i) of a band: what an XCD's L2 (4 MB) has to keep
                                   // from one level of a block to the next is rows x columns cells of Lwet3D / v3D / rho; with whole rows of 3600 cells
                                   // (0.1 degree) every line above / below came from HBM again (fetch 70 GB for 49 GB of touched inputs, profiles/r04 section 10)
#endif

// ---- march order of the fill pass's tiles (otmb_ctx_set_tile_order) -----------------------------------------------
// Tiles are 256 consecutive wet columns, i.e. pieces of one level's rows.  In wet-rank order a tile's vertical
// neighbours (levels k-1 and k+1 of Lwet3D, v3D, ρ) were touched one whole LEVEL of traffic earlier -- 124 MB of inputs
// plus 300 MB of outputs on a 1440x1080 grid, past every cache -- so they come from HBM three times.  In march order the
// tiles of a band of R rows are taken level after level: the same lines are needed again a few tiles later and are
// served by the L2 / Infinity Cache.  Bucket = (band, block of columns, level) -- one block per band unless the rows are longer than
// OTMB_MARCH_AUTO_COLS cells; a tile belongs to the block its first cell lies in -- ; a counting sort of the tiles by bucket.  Speed only.
__device__ __forceinline__ unsigned order_key(const i64 *__restrict__ lwet, i64 t, i64 n, int nx, int ny, i64 P, int rows, int nz, int topo, int cols) {
    const i64 L = lwet[t * TM_THREADS] - 1;  // (whatever Lwet holds, the key stays inside the bucket table)
    i64 k = L / P, j = (L - k * P) / nx;
    i64 ic = (L - k * P - j * nx) / cols;
    const i64 nblk = (nx + cols - 1) / cols;
    ic = ic < 0 ? 0 : (ic >= nblk ? nblk - 1 : ic);
    k = k < 0 ? 0 : (k >= nz ? nz - 1 : k);
    j = j < 0 ? 0 : (j >= ny ? ny - 1 : j);
    // HEAVY tiles -- bucket 0, the front of the sequence, dealt over the XCDs by xcd_position: tiles with cells on the tripolar
    // seam row (generic column builder, waves live about twice as long).  Lwet ascends, so the tile's cells lie between its
    // first and its last entry in (level, row) order: it touches row ny - 1 iff it starts there, ends there or runs into the next level.
    if (topo == OTMB_TRIPOLAR && nx >= 3) {
        const i64 wl = (t * TM_THREADS + TM_THREADS - 1 < n) ? t * TM_THREADS + TM_THREADS - 1 : n - 1;
        const i64 L1 = lwet[wl] - 1;
        i64 k1 = L1 / P, j1 = (L1 - k1 * P) / nx;
        if (j == ny - 1 || j1 == ny - 1 || k1 > k) return 0u;
    }
    // bands from north to south (the seam row's neighbours at the START of an XCD's eighth: -5 % at 1 degree against south first)
    return 1u + ((unsigned)((ny - 1 - j) / rows) * (unsigned)nblk + (unsigned)ic) * (unsigned)nz + (unsigned)k;
}
__global__ void order_hist(const i64 *__restrict__ lwet, i64 ntiles, i64 n, int nx, int ny, i64 P, int rows, int nz, int topo, int cols, unsigned *hist) {
    const i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < ntiles) atomicAdd(&hist[order_key(lwet, t, n, nx, ny, P, rows, nz, topo, cols)], 1u);
}
__global__ __launch_bounds__(1024) void order_scan(unsigned *hist, i64 nbuckets) {  // in place: exclusive prefix
    __shared__ unsigned wave_tot[16];
    __shared__ unsigned carry;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (i64 b0 = 0; b0 < nbuckets; b0 += 1024) {
        const i64 b = b0 + tid;
        const unsigned mine = (b < nbuckets) ? hist[b] : 0u;
        unsigned incl = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned y = __shfl_up(incl, d);
            if (lane >= d) incl += y;
        }
        if (lane == 63) wave_tot[wid] = incl;
        __syncthreads();
        unsigned before = carry;
        for (int q = 0; q < wid; ++q) before += wave_tot[q];
        if (b < nbuckets) hist[b] = before + incl - mine;
        __syncthreads();
        if (tid == 1023) carry = before + incl;
        __syncthreads();
    }
}
// every tile takes the next free position of its bucket: a bijection whatever the keys are (the order inside a bucket
// -- a few dozen neighbouring tiles -- is left to the atomics)
__global__ void order_scatter(const i64 *__restrict__ lwet, i64 ntiles, i64 n, int nx, int ny, i64 P, int rows, int nz, int topo, int cols,
                              unsigned *cursor, unsigned *order) {
    const i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < ntiles) order[atomicAdd(&cursor[order_key(lwet, t, n, nx, ny, P, rows, nz, topo, cols)], 1u)] = (unsigned)t;
}

// Decide and build the tile order of a fill launch of ntiles tiles (TmParams.nt_order).  *order: the device pointer (or NULL: wet-rank order);
// *nheavy: how many heavy tiles it starts with.
int32_t otmb_tm_build_tile_order(otmb_ctx *ctx, const otmb_tm_args &a, i64 ntiles, const unsigned **order, unsigned *nheavy) {
    *order = nullptr;
    *nheavy = 0;
    int rows = ctx->march_rows;
    if (rows < 0) rows = OTMB_MARCH_AUTO_ROWS;
    if (rows <= 0 || ntiles < 64 || ntiles >= (1ll << 31) - 16) return OTMB_OK;
    if (rows > a.ny) rows = (int)a.ny;
    // blocks of columns: equal pieces of a row, none longer than the limit (whole rows when they are short enough)
    int cols = ctx->march_cols;
    if (cols < 0) cols = OTMB_MARCH_AUTO_COLS;
    if (cols <= 0 || cols >= a.nx) cols = (int)a.nx;
    else { const i64 nb_ = (a.nx + cols - 1) / cols; cols = (int)((a.nx + nb_ - 1) / nb_); }
    const i64 nblk = (a.nx + cols - 1) / cols;
    const i64 nbands = (a.ny + rows - 1) / rows, nbuckets = nbands * nblk * a.nz + 1;
    if (nbuckets >= (1ll << 31)) return OTMB_OK;
    const size_t ob = ((size_t)ntiles * sizeof(unsigned) + 255) / 256 * 256, bb = ((size_t)nbuckets * sizeof(unsigned) + 255) / 256 * 256;
    // the order is a function of the grid alone: computed once per (Lwet array, shape, band height) and kept.  (Any permutation of
    // the tiles is correct, so an Lwet array rewritten in place can only cost speed.)
    otmb_ctx::OrderKey key;
    key.lwet = a.lwet; key.n = a.n_wet; key.nx = a.nx; key.ny = a.ny; key.nz = a.nz; key.rows = rows; key.topo = a.topology; key.cols = cols;
    if (ctx->order.p && ctx->order.cap >= ob + bb && ctx->order_key == key) {
        *order = (const unsigned *)ctx->order.p;
        *nheavy = ctx->deal_heavy ? ctx->order_nheavy : 0u;
        return OTMB_OK;
    }
    int32_t rc;
    // (a failed or half-enqueued build must not be trusted by the next call: the key is recorded only once all three kernels are
    // enqueued without an error, on the stream they were enqueued on -- otmb_ctx_set_stream forgets the key, so a fill on another
    // stream can never read a permutation that is still being built)
    ctx->order_key = otmb_ctx::OrderKey();
    if ((rc = otmb_reserve(ctx, ctx->order, ob + bb))) return rc;
    unsigned *perm = (unsigned *)ctx->order.p, *hist = (unsigned *)((char *)ctx->order.p + ob);
    {
        KernelTimer kt(ctx, K_TM_ORDER);
        HIP_TRY(ctx, hipMemsetAsync(hist, 0, bb, ctx->stream));
        const unsigned nb = (unsigned)((ntiles + 255) / 256);
        hipLaunchKernelGGL(order_hist, dim3(nb), dim3(256), 0, ctx->stream, (const i64 *)a.lwet, ntiles, (i64)a.n_wet, (int)a.nx, (int)a.ny, a.nx * a.ny,
                           rows, (int)a.nz, (int)a.topology, cols, hist);
        hipLaunchKernelGGL(order_scan, dim3(1), dim3(1024), 0, ctx->stream, hist, nbuckets);
        // the number of heavy tiles = the exclusive prefix at bucket 1: the host needs it (grid size, kernel argument), once per grid
        HIP_TRY(ctx, hipMemcpyAsync(ctx->h_tot + 14, hist + 1, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
        hipLaunchKernelGGL(order_scatter, dim3(nb), dim3(256), 0, ctx->stream, (const i64 *)a.lwet, ntiles, (i64)a.n_wet, (int)a.nx, (int)a.ny, a.nx * a.ny,
                           rows, (int)a.nz, (int)a.topology, cols, hist, perm);
    }
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    unsigned nh = *(const unsigned *)(ctx->h_tot + 14);
    if (nh > (unsigned)ntiles) nh = 0;  // (cannot happen; any value <= ntiles is a correct mapping)
    ctx->order_nheavy = nh;
    ctx->order_key = key;
    *order = perm;
    *nheavy = ctx->deal_heavy ? nh : 0u;
    return OTMB_OK;
}
