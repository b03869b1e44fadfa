// Launch interface of the sequence-packing kernels (pack.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace tkz {

constexpr uint32_t PACK_NO_ID = 0xFFFFFFFFu;  // TKZ_NO_ID
constexpr uint32_t PACK_TILE = 2048;          // stream positions one block emits per step

// tkz_pack_params, validated by the caller (seq_len >= 1, id_width 2 or 4, ids that fit it)
struct PackParams {
    uint64_t seq_len;
    uint32_t bos_id, eos_id;  // PACK_NO_ID: none
    uint32_t pad_id;
    int id_width;             // bytes per packed id: 4 or 2
};

// ceil((n_tokens + n_docs * k) / seq_len): the rows a stream of that many tokens fills
uint64_t pack_rows(const PackParams& P, uint64_t n_docs, uint64_t n_tokens);

// CSR (d_row[0..n_docs], d_ids) -> [n_rows, seq_len] rows of the document stream with
// BOS / EOS separators; no allocation, no host sync, asynchronous on st. d_out (id_width
// bytes per element, 16-byte aligned) holds rows_capacity rows; d_seg / d_pos (u32 per
// position) and d_doc_pos (u64[n_docs + 1]) may be null. d_counts[0] = n_rows, [1] = T;
// *d_status is set to `err` when n_rows > rows_capacity (only the first rows_capacity rows
// are written) or, with id_width 2, when an input id needs more than 16 bits.
hipError_t launch_pack(const PackParams& P, const uint64_t* d_row, const uint32_t* d_ids, uint64_t n_docs,
                       uint64_t rows_capacity, void* d_out, uint32_t* d_seg, uint32_t* d_pos, uint64_t* d_doc_pos,
                       uint64_t* d_counts, uint32_t* d_status, uint32_t err, hipStream_t st);

}  // namespace tkz
