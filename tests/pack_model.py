"""Numpy restatement of the sequence-packing contract (include/tkz.h, tkz_pack_params):
straight loops over the documents, written from the contract and not from pack.hip."""
import numpy as np

NO_ID = 0xFFFFFFFF


def pack_rows(n_docs, n_tokens, seq_len, bos_id=None, eos_id=None):
    k = (bos_id is not None) + (eos_id is not None)
    return -(-(int(n_tokens) + int(n_docs) * k) // int(seq_len))


def stream(row_ptr, ids, bos_id=None, eos_id=None):
    """The unpadded token stream: (ids, segment_ids, position_ids, doc_pos) as lists."""
    row_ptr = [int(x) for x in row_ptr]
    ids = [int(x) for x in ids]
    out_ids, seg, pos, doc_pos = [], [], [], []
    for d in range(len(row_ptr) - 1):
        doc_pos.append(len(out_ids))
        j = 0
        if bos_id is not None:
            out_ids.append(bos_id); seg.append(d); pos.append(j); j += 1
        for t in range(row_ptr[d], row_ptr[d + 1]):
            out_ids.append(ids[t]); seg.append(d); pos.append(j); j += 1
        if eos_id is not None:
            out_ids.append(eos_id); seg.append(d); pos.append(j); j += 1
    doc_pos.append(len(out_ids))
    return out_ids, seg, pos, doc_pos


def rows(st, seq_len, pad_id=0, dtype=np.uint32):
    """Cuts a stream() into [n_rows, seq_len] rows, the tail of the last row padded."""
    out_ids, seg, pos, doc_pos = st
    L, T = int(seq_len), len(out_ids)
    n_rows = -(-T // L)
    tail = n_rows * L - T
    return {"ids": np.array(out_ids + [pad_id] * tail, dtype=np.uint64).astype(dtype).reshape(n_rows, L),
            "segment_ids": np.array(seg + [NO_ID] * tail, dtype=np.uint32).reshape(n_rows, L),
            "position_ids": np.array(pos + [0] * tail, dtype=np.uint32).reshape(n_rows, L),
            "doc_pos": np.array(doc_pos, dtype=np.uint64), "n_tokens": T, "n_rows": n_rows}


def pack(row_ptr, ids, seq_len, bos_id=None, eos_id=None, pad_id=0, dtype=np.uint32):
    """-> {"ids", "segment_ids", "position_ids"} of shape [n_rows, seq_len], "doc_pos"
    u64[n_docs + 1], "n_tokens" (T) and "n_rows"."""
    return rows(stream(row_ptr, ids, bos_id, eos_id), seq_len, pad_id, dtype)
