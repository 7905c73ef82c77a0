// otmb_prims.h -- how this library scans, sorts and sizes sort keys, and the small plumbing the sparse utilities share (sparse(), lump_and_spray,
// coarsen, the operator plan, submatrix, set_lines): launch shapes, widening and iota, scratch that frees itself, staging offsets.
// Declarations only; otmb_prims.hip is the one file of the library that includes rocPRIM.
#pragma once
#include <deque>

#include "otmb_common.h"

// ---- scan: out[i] = in[0] + ... + in[i - 1] (exclusive; out[0] = 0) or ... + in[i] (inclusive), i < n, on ctx->stream.
// tmp: the caller's buffer for rocPRIM's temporary, grown to what this call needs (never below 16 bytes, so a floor of otmb_reserve_some is moot).
int32_t otmb_exclusive_scan(otmb_ctx *ctx, DevBuf &tmp, const i64 *in, i64 *out, i64 n);
int32_t otmb_inclusive_scan(otmb_ctx *ctx, DevBuf &tmp, const i64 *in, i64 *out, i64 n);

// ---- sort: stable LSD radix sort of n (key, value) pairs over key bits [0, bits), on ctx->stream; tmp as above.
// (The u64 inputs are not const: that is the instantiation sparse() and coarsen have always shared.)
int32_t otmb_sort_pairs(otmb_ctx *ctx, DevBuf &tmp, u64 *keys_in, u64 *keys_out, u64 *vals_in, u64 *vals_out, i64 n, int bits);
int32_t otmb_sort_pairs(otmb_ctx *ctx, DevBuf &tmp, const i64 *keys_in, i64 *keys_out, const i64 *vals_in, i64 *vals_out, i64 n, int bits);
int32_t otmb_sort_pairs(otmb_ctx *ctx, DevBuf &tmp, const unsigned *keys_in, unsigned *keys_out, const i64 *vals_in, i64 *vals_out, i64 n, int bits);

// bits a value needs in a sort key: the smallest b >= 1 with v < 2^b, at most 63 (v >= 0)
static inline int otmb_bits(i64 v) {
    int b = 1;
    while (b < 63 && (v >> b) != 0) ++b;
    return b;
}

// ---- 1-D launch shapes of 256 threads, never an empty grid: <<<OTMB_GRID...(n, stream)>>>
// capped at 65536 workgroups: for grid-stride kernels
#define OTMB_GRID_STRIDE(n, st) dim3((unsigned)(((n) + 255) / 256 < 65536 ? (((n) + 255) / 256 > 0 ? ((n) + 255) / 256 : 1) : 65536)), dim3(256), 0, st
// exact: for kernels of one thread per element
#define OTMB_GRID_EXACT(n, st) dim3((unsigned)(((n) + 255) / 256 > 0 ? ((n) + 255) / 256 : 1)), dim3(256), 0, st

// ---- element kernels (one launch each, n == 0 included): out[q] = in[q] + add and a[q] = first + q, q < n
void otmb_widen(hipStream_t st, const uint8_t *in, i64 n, i64 add, i64 *out);
void otmb_widen(hipStream_t st, const unsigned *in, i64 n, i64 add, i64 *out);
void otmb_widen(hipStream_t st, const int *in, i64 n, i64 add, i64 *out);
void otmb_iota(hipStream_t st, i64 *a, i64 n, i64 first);

// otmb_reserve for arrays that may be empty: a null pointer is never handed to a kernel
static inline int32_t otmb_reserve_some(otmb_ctx *ctx, DevBuf &b, size_t bytes) { return otmb_reserve(ctx, b, bytes > 0 ? bytes : 8); }
static inline void otmb_free(DevBuf &b) {
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.cap = 0;
}

// ---- device scratch of one call, freed on every return (hipFree waits for the kernels that use it); add() hands out references that stay valid
struct DevScratch {
    std::deque<DevBuf> bufs;
    DevBuf &add() { return bufs.emplace_back(); }
    DevScratch() = default;
    DevScratch(const DevScratch &) = delete;
    DevScratch &operator=(const DevScratch &) = delete;
    ~DevScratch() {
        for (DevBuf &b : bufs) otmb_free(b);
    }
};

// ---- offsets of the arrays a host-pointer entry point stages in ONE allocation, each on a 256-byte boundary
struct DevArena {
    size_t off = 0;
    size_t take(size_t bytes) {
        const size_t o = off;
        off += (bytes + 255) & ~(size_t)255;
        return o;
    }
    size_t total() const { return off; }
};
