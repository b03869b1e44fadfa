"""Sequence packing on the GPU (pack.hip through tkz_pack_batch_device, tkz_encode_pack_batch
and their Python mirrors) against the numpy model of the contract (tests/pack_model.py).
Every comparison is exact, and every output buffer carries a 256-byte canary behind
n_rows * seq_len elements that must come back unchanged."""
import ctypes
import json
import random

import numpy as np
import pytest

import tkz
from tkz import synth
from tests import pack_model as pm

pytestmark = pytest.mark.gpu

CFG = {"model": {"type": "WordPiece", "vocab": {"[UNK]": 0, "a": 1, "b": 2, "##b": 3, "ab": 4, "[PAD]": 5}},
       "pre_tokenizer": {"type": "Whitespace"}}
CANARY = 256
FILL = 0xA5
SEPS = {"none": (None, None), "bos": (60001, None), "eos": (None, 60002), "both": (60001, 60002)}
INVALID = 10


@pytest.fixture(scope="module")
def tok():
    t = tkz.Tokenizer.from_json(json.dumps(CFG))
    yield t
    t.close()


def _filled(nbytes):
    buf = tkz.DeviceBuffer(nbytes)
    buf.upload(np.full(nbytes, FILL, dtype=np.uint8))
    return buf


def device_pack(tok, row_ptr, ids, seq_len, bos=None, eos=None, pad=0, dtype=np.uint32, cap_rows=None,
                optional=True):
    """One tkz_pack_batch_device call on uploaded CSR arrays. Returns the raw outputs cut at
    the capacity, the counts, the status, and whether every canary survived."""
    row_ptr = np.ascontiguousarray(row_ptr, dtype=np.uint64)
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    n_docs = len(row_ptr) - 1
    n_tok = int(row_ptr[-1] - row_ptr[0])
    p = tkz.pack_params(seq_len, bos, eos, pad, dtype)
    if cap_rows is None:
        cap_rows = int(tkz.lib().tkz_pack_rows(ctypes.byref(p), n_docs, n_tok))
    w = np.dtype(dtype).itemsize
    n_pos = cap_rows * seq_len
    d_row, d_ids = tkz.DeviceBuffer(row_ptr.nbytes), tkz.DeviceBuffer(max(ids.nbytes, 16))
    d_row.upload(row_ptr)
    if ids.size:
        d_ids.upload(ids)
    d_out = _filled(n_pos * w + CANARY)
    d_seg = _filled(n_pos * 4 + CANARY) if optional else None
    d_pos = _filled(n_pos * 4 + CANARY) if optional else None
    d_doc = _filled((n_docs + 1) * 8 + CANARY) if optional else None
    d_cnt, d_st = _filled(16 + CANARY), tkz.DeviceBuffer(16)
    d_st.zero()
    rc = tkz.lib().tkz_pack_batch_device(tok.handle, d_row.ptr, d_ids.ptr, n_docs, ctypes.byref(p), cap_rows,
                                         d_out.ptr, d_seg.ptr if optional else None,
                                         d_pos.ptr if optional else None, d_doc.ptr if optional else None,
                                         d_cnt.ptr, d_st.ptr, None)
    assert rc == 0, tkz.lib().tkz_last_error()
    assert tkz.lib().tkz_synchronize(tok.handle) == 0
    res = {"canary": True}

    def fetch(buf, n_elems, dt):
        raw = buf.download(np.zeros(buf.nbytes, dtype=np.uint8))
        body = n_elems * np.dtype(dt).itemsize
        if not np.all(raw[body:body + CANARY] == FILL):
            res["canary"] = False
        return raw, raw[:body].view(dt)
    res["raw_ids"], res["ids"] = fetch(d_out, n_pos, dtype)
    if optional:
        _, res["segment_ids"] = fetch(d_seg, n_pos, np.uint32)
        _, res["position_ids"] = fetch(d_pos, n_pos, np.uint32)
        _, res["doc_pos"] = fetch(d_doc, n_docs + 1, np.uint64)
    _, res["counts"] = fetch(d_cnt, 2, np.uint64)
    res["status"] = int(d_st.download(np.zeros(4, dtype=np.uint32))[0])
    for b in (d_row, d_ids, d_out, d_seg, d_pos, d_doc, d_cnt, d_st):
        if b is not None:
            b.free()
    return res


def check(res, model, seq_len, what):
    """The device outputs of a full-capacity call equal the model's rows."""
    assert res["status"] == 0, what
    assert res["counts"].tolist() == [model["n_rows"], model["n_tokens"]], what
    assert res["canary"], what
    n = model["n_rows"] * seq_len
    assert np.array_equal(res["ids"][:n], model["ids"].ravel()), what
    if "segment_ids" in res:
        for k in ("segment_ids", "position_ids"):
            assert np.array_equal(res[k][:n], model[k].ravel()), (what, k)
        assert np.array_equal(res["doc_pos"], model["doc_pos"]), what


# ---- 1. a synthetic CSR with every kind of doc, crossed with seq_len / separators / width ----
def _mixed_lengths():
    rng = random.Random(20250)
    def mix(n):
        return [0 if rng.random() < 0.3 else rng.randint(1, 40) for _ in range(n)]
    lens = [0] * 310 + mix(700) + [rng.randint(5000, 20000) for _ in range(3)] + mix(500) + [0] * 330 + mix(400)
    lens += [rng.randint(5000, 20000) for _ in range(4)] + mix(400) + [17] + [0] * 305
    return lens


@pytest.fixture(scope="module")
def mixed():
    lens = _mixed_lengths()
    assert 2800 <= len(lens) <= 3300 and 100_000 <= sum(lens) <= 200_000
    row = np.zeros(len(lens) + 1, dtype=np.uint64)
    row[1:] = np.cumsum(lens)
    rng = np.random.default_rng(7)
    ids16 = rng.integers(0, 60000, size=int(row[-1]), dtype=np.uint32)
    ids32 = ids16 + rng.integers(0, 2, size=ids16.size, dtype=np.uint32) * np.uint32(0x7FFF0000)
    return {"row": row, 2: ids16, 4: ids32, "streams": {}}


def _stream(mixed, sep, width):
    key = (sep, width)
    if key not in mixed["streams"]:  # computed once, shared by every seq_len
        mixed["streams"][key] = pm.stream(mixed["row"], mixed[width], *SEPS[sep])
    return mixed["streams"][key]


@pytest.mark.parametrize("width", [4, 2])
@pytest.mark.parametrize("sep", sorted(SEPS))
def test_mixed_csr(tok, mixed, sep, width):
    st = _stream(mixed, sep, width)
    dtype = np.uint32 if width == 4 else np.uint16
    bos, eos = SEPS[sep]
    T = len(st[0])
    for L in (1, 7, 64, 129, 4099, T + 5):
        model = pm.rows(st, L, pad_id=59999, dtype=dtype)
        res = device_pack(tok, mixed["row"], mixed[width], L, bos, eos, 59999, dtype)
        check(res, model, L, (sep, width, L))


def test_sub_range_of_a_larger_csr(tok, mixed):
    row = mixed["row"][400:1600]  # row_ptr[0] != 0; ends inside the middle run of empty docs
    assert row[0] != 0
    model = pm.pack(row, mixed[4], 129, 60001, 60002, 3)
    res = device_pack(tok, row, mixed[4], 129, 60001, 60002, 3)
    check(res, model, 129, "sub-range")


# ---- 2. doc boundaries against tile boundaries ----
def _sweep_lengths():
    tile = int(tkz.lib().tkz_pack_tile())
    return [1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, tile - 1, tile, tile + 1]


@pytest.mark.parametrize("seps", [(None, None), (60001, 60002)])
def test_equal_length_docs_across_tiles(tok, seps):
    tile = int(tkz.lib().tkz_pack_tile())
    k = sum(s is not None for s in seps)
    rng = np.random.default_rng(11)
    for m in _sweep_lengths():
        n_docs = -(-3 * tile // (m + k)) + 2  # at least three tiles
        row = np.arange(n_docs + 1, dtype=np.uint64) * np.uint64(m)
        ids = rng.integers(0, 60000, size=int(row[-1]), dtype=np.uint32)
        for L, dtype in ((257, np.uint32), (tile, np.uint16)):
            model = pm.pack(row, ids, L, seps[0], seps[1], 9, dtype)
            assert model["n_tokens"] >= 3 * tile
            check(device_pack(tok, row, ids, L, seps[0], seps[1], 9, dtype), model, L, (m, seps, L))


def test_one_empty_doc_on_every_position(tok):
    tile = int(tkz.lib().tkz_pack_tile())
    n_docs = 3 * tile + 77
    row = np.full(n_docs + 1, 5, dtype=np.uint64)
    ids = np.arange(8, dtype=np.uint32)
    for L in (100, tile + 1):
        model = pm.pack(row, ids, L, None, 60002, 4)
        assert model["n_tokens"] == n_docs
        check(device_pack(tok, row, ids, L, None, 60002, 4), model, L, L)


# ---- 3. degenerate shapes ----
def test_no_docs_and_all_empty(tok):
    for row in (np.zeros(1, dtype=np.uint64), np.zeros(1001, dtype=np.uint64)):
        for dtype in (np.uint32, np.uint16):
            res = device_pack(tok, row, np.zeros(0, np.uint32), 16, None, None, 0, dtype, cap_rows=4)
            assert res["status"] == 0 and res["counts"].tolist() == [0, 0] and res["canary"]
            assert np.all(res["raw_ids"] == FILL)  # nothing at all was written
            assert np.all(res["segment_ids"].view(np.uint8) == FILL)
            assert np.array_equal(res["doc_pos"], np.zeros(len(row), dtype=np.uint64))
    row = np.full(1001, 3, dtype=np.uint64)
    model = pm.pack(row, np.zeros(3, np.uint32), 16, None, 60002, 1)
    assert model["n_tokens"] == 1000
    check(device_pack(tok, row, np.zeros(3, np.uint32), 16, None, 60002, 1), model, 16, "all empty + eos")
    res = device_pack(tok, np.zeros(1, dtype=np.uint64), np.zeros(0, np.uint32), 16, 60001, 60002)
    assert res["counts"].tolist() == [0, 0] and res["status"] == 0 and res["canary"]


# ---- 4. device-detected errors ----
def test_capacity_one_row_short(tok, mixed):
    row, ids = mixed["row"][:900], mixed[4]
    model = pm.pack(row, ids, 129, 60001, None, 0)
    for dtype in (np.uint32, np.uint16):
        res = device_pack(tok, row, mixed[2], 129, 60001, None, 0, dtype, cap_rows=model["n_rows"] - 1)
        assert res["status"] == INVALID
        assert res["counts"].tolist() == [model["n_rows"], model["n_tokens"]]
        assert res["canary"]  # nothing past the capacity
    res = device_pack(tok, row, ids, 129, 60001, None, 0, cap_rows=0)
    assert res["status"] == INVALID and res["canary"] and np.all(res["raw_ids"] == FILL)


def test_wide_id_in_two_byte_mode(tok):
    row = np.array([0, 3, 3, 5000], dtype=np.uint64)
    ids = np.full(5000, 7, dtype=np.uint32)
    assert device_pack(tok, row, ids, 64, dtype=np.uint16)["status"] == 0
    ids[4321] = 65536
    res = device_pack(tok, row, ids, 64, dtype=np.uint16)
    assert res["status"] == INVALID and res["canary"]
    check(device_pack(tok, row, ids, 64), pm.pack(row, ids, 64), 64, "4-byte ids take it")


# ---- 5. end to end ----
def _e2e(tok, data, off, L, bos, eos, pad):
    row, ids, _ = tok.encode_batch(data, off)
    for dtype in (np.uint32, np.uint16):
        model = pm.pack(row, ids, L, bos, eos, pad, dtype)
        got = tok.encode_pack(data, off, L, bos, eos, pad, dtype, segments=True, positions=True, doc_pos=True)
        assert got["n_tokens"] == model["n_tokens"] and got["ids"].dtype == np.dtype(dtype)
        for k in ("ids", "segment_ids", "position_ids", "doc_pos"):
            assert got[k].shape == model[k].shape and np.array_equal(got[k], model[k]), (dtype, k)
        plain = tok.encode_pack(data, off, L, bos, eos, pad, dtype)
        assert sorted(plain) == ["ids", "n_tokens"] and np.array_equal(plain["ids"], model["ids"])
    return row, ids


def test_encode_pack_c1():
    t = tkz.Tokenizer.from_json(synth.tokenizer_json(1))
    data, off = synth.docs(1, 256)
    _e2e(t, data, off, 512, 1, 2, 0)
    _e2e(t, data, off, 333, None, None, 7)
    t.close()


def _wordpiece_docs():
    rng = random.Random(5)
    words = [b"a", b"b", b"ab", b"abb", b"ba", b"x"]
    docs = [b" ".join(rng.choice(words) for _ in range(rng.randint(0, 30))) if rng.random() > 0.25 else b""
            for _ in range(3000)]
    docs = [b""] * 40 + docs + [b"", b"a", b""]
    off = np.zeros(len(docs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(d) for d in docs])
    return np.frombuffer(b"".join(docs), dtype=np.uint8), off


def test_encode_pack_wordpiece_with_empty_docs_and_padding_refused():
    t = tkz.Tokenizer.from_json(json.dumps(CFG))
    data, off = _wordpiece_docs()
    _e2e(t, data, off, 100, None, 5, 5)
    _e2e(t, data, off, 64, 5, None, 0)
    t.set_padding(16, pad_id=5)
    with pytest.raises(tkz.TokenizerError) as e:
        t.encode_pack(data, off, 64)
    assert e.value.code == INVALID
    t.close()


def test_device_batch_pack_same_stream_then_reuse():
    t = tkz.Tokenizer.from_json(synth.tokenizer_json(1))
    data, off = synth.docs(1, 256)
    row, ids, _ = t.encode_batch(data, off)
    stream = tkz.lib().tkz_stream_create()
    assert stream
    batch = tkz.DeviceBatch(t, data, off)
    packed = tkz.PackedBatch(t, batch.n_docs, batch.total + 2 * batch.n_docs + 600, True, True, True)
    batch.run(stream)  # no sync before the pack: same stream
    batch.pack(600, 1, 2, 3, np.uint32, True, True, True, stream=stream, out=packed)
    got = packed.results()
    model = pm.pack(row, ids, 600, 1, 2, 3)
    assert got["n_tokens"] == model["n_tokens"]
    for k in ("ids", "segment_ids", "position_ids", "doc_pos"):
        assert np.array_equal(got[k], model[k]), k
    # a smaller batch into the same buffers, other parameters
    small = tkz.DeviceBatch(t, data[: int(off[100])], off[:101])
    small.run(stream)
    small.pack(77, None, 2, 9, np.uint16, True, False, False, stream=stream, out=packed)
    got = packed.results()
    model = pm.pack(row[:101], ids, 77, None, 2, 9, np.uint16)
    assert got["n_tokens"] == model["n_tokens"] < len(ids) and sorted(got) == ["ids", "n_tokens", "segment_ids"]
    assert np.array_equal(got["ids"], model["ids"]) and np.array_equal(got["segment_ids"], model["segment_ids"])
    # the default stream and buffers of pack()'s own
    own = batch.pack(512, dtype=np.uint16)
    assert np.array_equal(own.results()["ids"], pm.pack(row, ids, 512, dtype=np.uint16)["ids"])
    for b in (own, packed, small, batch):
        b.free()
    tkz.lib().tkz_stream_destroy(stream)
    t.close()
