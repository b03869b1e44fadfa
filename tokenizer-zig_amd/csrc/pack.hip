// MI355X (gfx950) sequence packing: a CSR batch of encodings -> the token stream a
// pre-training loader consumes. The docs are concatenated, each with an optional BOS in
// front and EOS behind (the batched counterpart of Encoding.mergeWith,
// jrc2139/tokenizer-zig src/encoding.zig:520-583), and the stream is cut every seq_len
// tokens into a dense [n_rows, seq_len] tensor of 4- or 2-byte ids, with optional segment
// (doc index) and position (index inside the doc's span) ids per position.
//
// Doc d starts at stream position s[d] = (row_ptr[d] - row_ptr[0]) + d * k, k = BOS + EOS:
// a closed form of row_ptr, so no scan and no workspace.
//   k_pack         — output-centric: a block owns a run of tiles of PACK_TILE consecutive
//                    positions. Per tile: one search of s[] for the doc of the first position
//                    (outwards from a guess: the last doc of the tile before), the doc starts
//                    inside the tile marked in LDS (max doc index per position: empty docs
//                    share one) and max-scanned so every position knows its doc, values
//                    gathered with position-major (coalesced) loads into LDS, then written
//                    with 16-byte stores.
//   k_pack_doc_pos — s[0..n_docs] as u64 (the stream's cu_seqlens).
// Every index is 64-bit (n_rows * seq_len can pass 2^32); doc indices are 32-bit, as the
// segment ids are.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pack.hpp"

namespace tkz {

constexpr int PACK_THREADS = 256;
constexpr int PACK_PER = PACK_TILE / PACK_THREADS;  // positions per thread in the scan
constexpr uint64_t PACK_RUN = 8;                    // consecutive tiles per block
constexpr unsigned PACK_MAX_BLOCKS = 1u << 30;
static_assert(PACK_PER == 8, "the scan and the 2-byte store read 8 positions per thread");

struct PackArgs {
    const uint64_t* row;
    const uint32_t* ids;
    uint64_t n_docs;
    uint64_t L, cap_rows;
    uint64_t run;  // consecutive tiles per block
    uint32_t bos, eos, pad;
    uint32_t kb, ke;
    void* out;
    uint32_t* seg;
    uint32_t* pos;
    uint64_t* counts;
    uint32_t* status;
    uint32_t err;
};

__device__ __forceinline__ uint64_t doc_start(const uint64_t* __restrict__ row, uint64_t base, uint64_t k,
                                              uint64_t d) {
    return row[d] - base + d * k;
}

// The largest d in [0, n_docs) with s[d] <= p (p < T, so there is one), searched outwards
// from a guess g < n_docs: doubling steps up or down until the doc is bracketed, then a
// bisection, so the cost is the logarithm of the guess's error. Block-uniform (every
// thread runs the same loads).
__device__ uint64_t find_doc(const uint64_t* __restrict__ row, uint64_t base, uint64_t k, uint64_t n_docs,
                             uint64_t g, uint64_t p) {
    uint64_t lo, hi, step = 1;  // s[lo] <= p, and s[hi] > p or hi == n_docs
    if (doc_start(row, base, k, g) <= p) {
        lo = g;
        hi = g + 1;
        while (hi < n_docs && doc_start(row, base, k, hi) <= p) {
            lo = hi;
            step <<= 1;
            hi = (n_docs - lo > step) ? lo + step : n_docs;
        }
    } else {
        hi = g;
        lo = g - 1;  // (g > 0: s[0] = 0 <= p)
        while (doc_start(row, base, k, lo) > p) {  // ends at lo == 0 at the latest
            hi = lo;
            step <<= 1;
            lo = lo > step ? lo - step : 0;
        }
    }
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (doc_start(row, base, k, mid) <= p) lo = mid; else hi = mid;
    }
    return lo;
}

// PACK_TILE u32 values of LDS -> dst[p0 ...) below lim, 4 per lane and store.
__device__ __forceinline__ void store_tile_u32(uint32_t* __restrict__ dst, const uint32_t* src, uint64_t p0,
                                               uint64_t lim, int tid) {
#pragma unroll
    for (int c = 0; c < PACK_TILE / (PACK_THREADS * 4); ++c) {
        const uint32_t b = (uint32_t)(c * PACK_THREADS + tid) * 4;
        const uint64_t p = p0 + b;
        if (p + 4 <= lim) {
            *reinterpret_cast<uint4*>(dst + p) = *reinterpret_cast<const uint4*>(src + b);
        } else {
            for (uint32_t e = 0; e < 4; ++e)
                if (p + e < lim) dst[p + e] = src[b + e];
        }
    }
}

// The same as 2-byte ids, 8 per lane and store.
__device__ __forceinline__ void store_tile_u16(uint16_t* __restrict__ dst, const uint32_t* src, uint64_t p0,
                                               uint64_t lim, int tid) {
    const uint32_t b = (uint32_t)tid * 8;
    const uint64_t p = p0 + b;
    if (p + 8 <= lim) {
        const uint4 a = *reinterpret_cast<const uint4*>(src + b);
        const uint4 c = *reinterpret_cast<const uint4*>(src + b + 4);
        uint4 v;
        v.x = (a.x & 0xFFFFu) | (a.y << 16);
        v.y = (a.z & 0xFFFFu) | (a.w << 16);
        v.z = (c.x & 0xFFFFu) | (c.y << 16);
        v.w = (c.z & 0xFFFFu) | (c.w << 16);
        *reinterpret_cast<uint4*>(dst + p) = v;
    } else {
        for (uint32_t e = 0; e < 8; ++e)
            if (p + e < lim) dst[p + e] = (uint16_t)src[b + e];
    }
}

constexpr uint32_t PACK_ST_MASK = 0xFFFu;   // s_st: 1 + the tile offset of the doc's start (0: before the tile)
constexpr uint32_t PACK_ST_ENDS = 1u << 13;  // s_st: the next position begins another doc, or is T
static_assert(PACK_TILE < PACK_ST_MASK, "a start offset + 1 must fit PACK_ST_MASK");

template <bool W16>
__global__ __launch_bounds__(PACK_THREADS, 5) void k_pack(PackArgs A) {
    __shared__ __attribute__((aligned(16))) uint32_t s_doc[PACK_TILE];  // doc starts -> doc of each position -> segment id
    __shared__ __attribute__((aligned(16))) uint32_t s_st[PACK_TILE];   // start of each position's doc -> position id
    __shared__ __attribute__((aligned(16))) uint32_t s_val[PACK_TILE];
    __shared__ uint32_t s_wave[2][PACK_THREADS / 64];
    __shared__ uint32_t s_next;  // a doc starts at the first position behind the tile
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t* __restrict__ row = A.row;
    const uint64_t n_docs = A.n_docs, L = A.L;
    const uint64_t base = row[0], end_all = row[n_docs];
    const uint64_t k = (uint64_t)A.kb + A.ke;
    const uint64_t T = end_all - base + n_docs * k;
    const uint64_t n_rows = T / L + (T % L ? 1 : 0);
    if (blockIdx.x == 0 && tid == 0) {
        A.counts[0] = n_rows;
        A.counts[1] = T;
        if (n_rows > A.cap_rows) *A.status = A.err;
    }
    const uint64_t lim = (n_rows < A.cap_rows ? n_rows : A.cap_rows) * L;  // positions written
    const uint64_t n_tiles = lim / PACK_TILE + (lim % PACK_TILE ? 1 : 0);
    uint64_t tile = (uint64_t)blockIdx.x * A.run;
    const uint64_t tile_end = tile + A.run < n_tiles ? tile + A.run : n_tiles;
    // the block's first search starts where docs of equal length would put the position;
    // every later one at the last doc of the tile before
    uint64_t hint = 0;
    if (tile < tile_end && tile * PACK_TILE < T) {
        hint = (uint64_t)((double)(tile * PACK_TILE) / (double)T * (double)n_docs);
        if (hint >= n_docs) hint = n_docs - 1;
    }
    bool bad = false;
    for (; tile < tile_end; ++tile) {
        const uint64_t p0 = tile * PACK_TILE;
        const uint64_t doc_end = p0 + PACK_TILE < T ? p0 + PACK_TILE : T;  // doc positions: [p0, doc_end)
        // stream positions of the tile, (far) more than PACK_TILE when T is behind it, so the
        // last position of the stream ends its doc and that of a full tile need not
        const uint32_t n_in = p0 >= T ? 0u : (T - p0 <= PACK_TILE ? (uint32_t)(T - p0) : ~0u);
        uint64_t d0 = 0, sd0 = 0;  // the doc that holds p0 and its start
        if (p0 < T) {
            d0 = find_doc(row, base, k, n_docs, hint, p0);
            sd0 = doc_start(row, base, k, d0);
        }
#pragma unroll
        for (int c = 0; c < PACK_PER; ++c) s_doc[c * PACK_THREADS + tid] = 0;
        if (tid == 0) s_next = 0;
        __syncthreads();
        // the docs that start inside the tile (d0 holds p0, so they start past it). The first
        // doc at doc_end or beyond ends the walk (with k == 0 the empty docs at T hold no
        // position) and tells whether the tile's last position is the last of its doc
        if (p0 < T) {
            for (uint64_t d = d0 + 1 + (uint64_t)tid; d < n_docs; d += PACK_THREADS) {
                const uint64_t sd = doc_start(row, base, k, d);
                if (sd >= doc_end) {
                    if (sd == p0 + PACK_TILE) s_next = 1;
                    break;
                }
                if (sd >= p0) atomicMax(&s_doc[sd - p0], (uint32_t)(d - d0));
            }
        }
        __syncthreads();
        // block-wide inclusive max-scans over the marks: position -> its doc (relative to d0)
        // and 1 + the offset that doc starts at (0: d0, which starts at sd0)
        uint32_t m[PACK_PER], st[PACK_PER];
        uint32_t starts = 0;  // bit i: a doc starts at this thread's position i (bit PACK_PER: the next thread's first)
        {
            const uint4 a = *reinterpret_cast<const uint4*>(&s_doc[tid * PACK_PER]);
            const uint4 b = *reinterpret_cast<const uint4*>(&s_doc[tid * PACK_PER + 4]);
            m[0] = a.x; m[1] = a.y; m[2] = a.z; m[3] = a.w;
            m[4] = b.x; m[5] = b.y; m[6] = b.z; m[7] = b.w;
            const uint32_t nxt = tid + 1 < PACK_THREADS ? s_doc[(tid + 1) * PACK_PER] : s_next;
            if (nxt) starts |= 1u << PACK_PER;
        }
#pragma unroll
        for (int i = 0; i < PACK_PER; ++i) {
            if (m[i]) starts |= 1u << i;
            st[i] = m[i] ? (uint32_t)(tid * PACK_PER + i + 1) : 0u;
        }
#pragma unroll
        for (int i = 1; i < PACK_PER; ++i) {
            m[i] = m[i] > m[i - 1] ? m[i] : m[i - 1];
            st[i] = st[i] > st[i - 1] ? st[i] : st[i - 1];
        }
        uint32_t inc = m[PACK_PER - 1], inc_st = st[PACK_PER - 1];
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t v = __shfl_up(inc, o), vs = __shfl_up(inc_st, o);
            if (lane >= o && v > inc) inc = v;
            if (lane >= o && vs > inc_st) inc_st = vs;
        }
        if (lane == 63) {
            s_wave[0][wave] = inc;
            s_wave[1][wave] = inc_st;
        }
        __syncthreads();
        uint32_t ex = __shfl_up(inc, 1), ex_st = __shfl_up(inc_st, 1);
        if (lane == 0) ex = ex_st = 0;
        uint32_t last = 0;  // the tile's last doc
        for (int w = 0; w < PACK_THREADS / 64; ++w) {
            const uint32_t t = s_wave[0][w], ts = s_wave[1][w];
            if (w < wave && t > ex) ex = t;
            if (w < wave && ts > ex_st) ex_st = ts;
            if (t > last) last = t;
        }
        hint = d0 + last;
#pragma unroll
        for (int i = 0; i < PACK_PER; ++i) {
            m[i] = m[i] > ex ? m[i] : ex;
            st[i] = st[i] > ex_st ? st[i] : ex_st;
            if ((starts >> (i + 1) & 1u) || (uint32_t)(tid * PACK_PER + i + 1) == n_in) st[i] |= PACK_ST_ENDS;
        }
        *reinterpret_cast<uint4*>(&s_doc[tid * PACK_PER]) = uint4{m[0], m[1], m[2], m[3]};
        *reinterpret_cast<uint4*>(&s_doc[tid * PACK_PER + 4]) = uint4{m[4], m[5], m[6], m[7]};
        *reinterpret_cast<uint4*>(&s_st[tid * PACK_PER]) = uint4{st[0], st[1], st[2], st[3]};
        *reinterpret_cast<uint4*>(&s_st[tid * PACK_PER + 4]) = uint4{st[4], st[5], st[6], st[7]};
        __syncthreads();
        // values, position-major: consecutive lanes read consecutive ids of a doc. Position p
        // of doc d has d * k + kb separators before it, so its token is ids[base + p - d*k - kb]:
        // row_ptr is not read again. Two passes, so a thread's loads are in flight together
        // (per-position arithmetic is 32-bit, relative to the tile; only the id's index is not)
        const uint32_t j0 = (uint32_t)(p0 - sd0);          // position id of p0 in d0
        const uint64_t src0 = base + p0 - d0 * k - A.kb;   // ids index of p0, were it d0's token
        uint32_t tokv[PACK_PER];
        uint32_t is_bos = 0, is_eos = 0;
#pragma unroll
        for (int c = 0; c < PACK_PER; ++c) {
            const uint32_t i = (uint32_t)(c * PACK_THREADS + tid);
            const uint32_t w = s_st[i], o = w & PACK_ST_MASK, rel = s_doc[i];
            const bool in = i < n_in;
            const bool first = o ? i + 1 == o : (i == 0 && p0 == sd0);  // the first position of its doc
            const bool bos = in && A.kb && first, eos = in && A.ke && (w & PACK_ST_ENDS);
            const uint64_t src = src0 + i - (uint64_t)rel * k;
            s_doc[i] = in ? (uint32_t)d0 + rel : PACK_NO_ID;  // (each thread reads and writes its own i)
            s_st[i] = !in ? 0u : o ? i + 1 - o : j0 + i;
            if (bos) is_bos |= 1u << c;
            if (eos) is_eos |= 1u << c;
            tokv[c] = 0;
            if (in && !bos && !eos) {
                if (src < end_all) tokv[c] = A.ids[src]; else bad = true;  // (a row_ptr that is not monotone)
            }
        }
#pragma unroll
        for (int c = 0; c < PACK_PER; ++c) {
            const uint32_t i = (uint32_t)(c * PACK_THREADS + tid);
            const bool in = i < n_in;
            if (W16 && tokv[c] > 0xFFFFu) bad = true;
            s_val[i] = !in ? A.pad : (is_bos >> c & 1u) ? A.bos : (is_eos >> c & 1u) ? A.eos : tokv[c];
        }
        __syncthreads();
        if (W16) store_tile_u16((uint16_t*)A.out, s_val, p0, lim, tid);
        else store_tile_u32((uint32_t*)A.out, s_val, p0, lim, tid);
        if (A.seg) store_tile_u32(A.seg, s_doc, p0, lim, tid);
        if (A.pos) store_tile_u32(A.pos, s_st, p0, lim, tid);
        __syncthreads();
    }
    if (bad) *A.status = A.err;
}

__global__ __launch_bounds__(256) void k_pack_doc_pos(const uint64_t* __restrict__ row, uint64_t n_docs, uint64_t k,
                                                      uint64_t* __restrict__ doc_pos) {
    const uint64_t base = row[0];
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t d = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; d <= n_docs; d += stride)
        doc_pos[d] = row[d] - base + d * k;
}

uint64_t pack_rows(const PackParams& P, uint64_t n_docs, uint64_t n_tokens) {
    const uint64_t k = (P.bos_id != PACK_NO_ID) + (P.eos_id != PACK_NO_ID);
    const uint64_t T = n_tokens + n_docs * k;
    return T / P.seq_len + (T % P.seq_len ? 1 : 0);
}

hipError_t launch_pack(const PackParams& P, const uint64_t* d_row, const uint32_t* d_ids, uint64_t n_docs,
                       uint64_t rows_capacity, void* d_out, uint32_t* d_seg, uint32_t* d_pos, uint64_t* d_doc_pos,
                       uint64_t* d_counts, uint32_t* d_status, uint32_t err, hipStream_t st) {
    PackArgs A;
    A.row = d_row; A.ids = d_ids; A.n_docs = n_docs;
    A.L = P.seq_len; A.cap_rows = rows_capacity;
    A.bos = P.bos_id; A.eos = P.eos_id; A.pad = P.pad_id;
    A.kb = P.bos_id != PACK_NO_ID ? 1u : 0u;
    A.ke = P.eos_id != PACK_NO_ID ? 1u : 0u;
    A.out = d_out; A.seg = d_seg; A.pos = d_pos;
    A.counts = d_counts; A.status = d_status; A.err = err;
    if (d_doc_pos) {
        const uint64_t b = (n_docs + 1 + 255) / 256;
        hipLaunchKernelGGL(k_pack_doc_pos, dim3((unsigned)(b < 2048 ? b : 2048)), dim3(256), 0, st,
                           d_row, n_docs, (uint64_t)A.kb + A.ke, d_doc_pos);
    }
    // one block per run of PACK_RUN consecutive tiles of the capacity: the kernel reads the
    // real size on the device and the blocks past it exit. Many more blocks than the device
    // holds at once, so its CUs stay evenly loaded to the end
    const uint64_t cap_pos = rows_capacity * P.seq_len;
    const uint64_t tiles = cap_pos / PACK_TILE + (cap_pos % PACK_TILE ? 1 : 0);
    A.run = PACK_RUN;
    if ((tiles + A.run - 1) / A.run > PACK_MAX_BLOCKS) A.run = (tiles + PACK_MAX_BLOCKS - 1) / PACK_MAX_BLOCKS;
    const unsigned grid = tiles ? (unsigned)((tiles + A.run - 1) / A.run) : 1u;
    if (P.id_width == 2) hipLaunchKernelGGL(k_pack<true>, dim3(grid), dim3(PACK_THREADS), 0, st, A);
    else hipLaunchKernelGGL(k_pack<false>, dim3(grid), dim3(PACK_THREADS), 0, st, A);
    return hipGetLastError();
}

}  // namespace tkz
