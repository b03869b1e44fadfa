"""Sequence packing without a GPU: the numpy model of the contract (tests/pack_model.py)
against hand-written cases, tkz_pack_rows against the model, and every argument check of
tkz_pack_batch_device / tkz_encode_pack_batch, which must come back as InvalidArgument
before any device use (a machine without a GPU never sees DeviceError for them)."""
import ctypes
import json

import numpy as np
import pytest

import tkz
from tests import pack_model as pm

NO = pm.NO_ID
ROW = [0, 2, 2, 5]   # docs: [10, 11], [], [12, 13, 14]
IDS = [10, 11, 12, 13, 14]
CFG = {"model": {"type": "WordPiece", "vocab": {"[UNK]": 0, "a": 1, "b": 2, "##b": 3, "ab": 4, "[PAD]": 5}},
       "pre_tokenizer": {"type": "Whitespace"}}
INVALID = 10


def _flat(m):
    return m["ids"].ravel().tolist(), m["segment_ids"].ravel().tolist(), m["position_ids"].ravel().tolist()


def test_model_no_separators_empty_doc_holds_no_position():
    m = pm.pack(ROW, IDS, 4, pad_id=9)
    ids, seg, pos = _flat(m)
    assert m["ids"].shape == (2, 4) and m["n_tokens"] == 5
    assert ids == [10, 11, 12, 13, 14, 9, 9, 9]
    assert seg == [0, 0, 2, 2, 2, NO, NO, NO]
    assert pos == [0, 1, 0, 1, 2, 0, 0, 0]
    assert m["doc_pos"].tolist() == [0, 2, 2, 5]


def test_model_bos_only():
    m = pm.pack(ROW, IDS, 3, bos_id=1)
    ids, seg, pos = _flat(m)
    assert ids == [1, 10, 11, 1, 1, 12, 13, 14, 0]
    assert seg == [0, 0, 0, 1, 2, 2, 2, 2, NO]
    assert pos == [0, 1, 2, 0, 0, 1, 2, 3, 0]
    assert m["doc_pos"].tolist() == [0, 3, 4, 8] and m["n_tokens"] == 8


def test_model_eos_only():
    m = pm.pack(ROW, IDS, 8, eos_id=2)
    ids, seg, pos = _flat(m)
    assert ids == [10, 11, 2, 2, 12, 13, 14, 2]   # T == L: one full row, no padding
    assert seg == [0, 0, 0, 1, 2, 2, 2, 2]
    assert pos == [0, 1, 2, 0, 0, 1, 2, 3]
    assert m["n_rows"] == 1


def test_model_both_separators_and_empty_doc():
    m = pm.pack(ROW, IDS, 5, bos_id=1, eos_id=2, pad_id=7)
    ids, seg, pos = _flat(m)
    assert ids == [1, 10, 11, 2, 1, 2, 1, 12, 13, 14, 2, 7, 7, 7, 7]
    assert seg == [0, 0, 0, 0, 1, 1, 2, 2, 2, 2, 2, NO, NO, NO, NO]
    assert pos == [0, 1, 2, 3, 0, 1, 0, 1, 2, 3, 4, 0, 0, 0, 0]
    assert m["doc_pos"].tolist() == [0, 4, 6, 11]


def test_model_seq_len_one_and_longer_than_stream():
    m = pm.pack(ROW, IDS, 1)
    assert m["ids"].shape == (5, 1) and m["ids"].ravel().tolist() == IDS
    m = pm.pack(ROW, IDS, 11, pad_id=3)
    assert m["ids"].shape == (1, 11) and m["ids"].ravel().tolist() == IDS + [3] * 6
    assert m["segment_ids"].ravel().tolist()[5:] == [NO] * 6


def test_model_exact_multiple_sub_range_and_empty():
    m = pm.pack(ROW, IDS + [15], 2)  # (the extra id is outside row_ptr's range)
    assert m["ids"].tolist() == [[10, 11], [12, 13], [14, 0]]
    m = pm.pack([0, 2, 2, 6], IDS + [15], 3)
    assert m["ids"].tolist() == [[10, 11, 12], [13, 14, 15]] and m["n_rows"] == 2  # no padding
    m = pm.pack([2, 2, 5], IDS, 2, dtype=np.uint16)  # row_ptr[0] != 0
    assert m["ids"].dtype == np.uint16 and m["ids"].tolist() == [[12, 13], [14, 0]]
    assert m["doc_pos"].tolist() == [0, 0, 3]
    m = pm.pack([0, 0, 0], [], 4)
    assert m["ids"].shape == (0, 4) and m["n_tokens"] == 0
    m = pm.pack([0, 0, 0], [], 4, eos_id=2)
    assert m["ids"].tolist() == [[2, 2, 0, 0]]
    m = pm.pack([0], [], 4, bos_id=1)
    assert m["n_rows"] == 0 and m["doc_pos"].tolist() == [0]


def test_pack_params_default():
    p = tkz._PackParams()
    p.seq_len = 1
    tkz.lib().tkz_pack_params_default(ctypes.byref(p))
    assert (p.seq_len, p.bos_id, p.eos_id, p.pad_id, p.id_width) == (2048, NO, NO, 0, 4)
    assert (p.want_segments, p.want_positions, p.want_doc_pos) == (0, 0, 0)
    assert tkz.lib().tkz_pack_tile() >= 256


@pytest.mark.parametrize("bos,eos", [(None, None), (1, None), (None, 2), (1, 2)])
def test_pack_rows_matches_model(bos, eos):
    L = tkz.lib()
    for n_docs, n_tok, sl in [(0, 0, 4), (3, 5, 4), (3, 5, 1), (3, 5, 5), (3, 5, 11), (7, 0, 3), (1000, 123457, 2048),
                              (1, 2 ** 33, 3), (5, 10, 2 ** 40)]:
        p = tkz.pack_params(sl, bos, eos)
        assert L.tkz_pack_rows(ctypes.byref(p), n_docs, n_tok) == pm.pack_rows(n_docs, n_tok, sl, bos, eos)
    row = np.array(ROW)
    for sl in (1, 2, 3, 4, 5, 6, 50):
        p = tkz.pack_params(sl, bos, eos)
        assert L.tkz_pack_rows(ctypes.byref(p), 3, 5) == pm.pack(row, IDS, sl, bos, eos)["n_rows"]
    assert L.tkz_pack_rows(None, 3, 5) == 0


def _wide_vocab_json():
    vocab = {"[UNK]": 0, "a": 1, "wide": 65536}
    return json.dumps({"model": {"type": "WordPiece", "vocab": vocab}, "pre_tokenizer": {"type": "Whitespace"}})


def _device_call(tok, p):
    """tkz_pack_batch_device with plausible (never dereferenced) pointers."""
    fake = ctypes.c_void_p(4096)
    return tkz.lib().tkz_pack_batch_device(tok.handle, fake, fake, 1, p, 1, fake, None, None, None, fake, fake, None)


def _host_call(tok, p):
    data = np.frombuffer(b"a b", dtype=np.uint8)
    off = np.array([0, 3], dtype=np.uint64)
    out = tkz._Packed()
    return tkz.lib().tkz_encode_pack_batch(tok.handle, data.ctypes.data_as(ctypes.c_void_p),
                                           off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), 1, p, ctypes.byref(out))


BAD_PARAMS = {
    "seq_len_0": dict(seq_len=0),
    "id_width_3": dict(seq_len=8, _width=3),
    "id_width_8": dict(seq_len=8, _width=8),
    "u16_bos": dict(seq_len=8, bos_id=65536, dtype=np.uint16),
    "u16_eos": dict(seq_len=8, eos_id=70000, dtype=np.uint16),
    "u16_pad": dict(seq_len=8, pad_id=65536, dtype=np.uint16),
}


@pytest.mark.parametrize("name", sorted(BAD_PARAMS))
@pytest.mark.parametrize("call", [_device_call, _host_call])
def test_invalid_params_fail_before_device_use(name, call):
    kw = dict(BAD_PARAMS[name])
    width = kw.pop("_width", None)
    p = tkz.pack_params(**kw)
    if width is not None:
        p.id_width = width
    tok = tkz.Tokenizer.from_json(json.dumps(CFG))
    assert call(tok, ctypes.byref(p)) == INVALID, name
    tok.close()


@pytest.mark.parametrize("call", [_device_call, _host_call])
def test_null_params_and_wide_vocab(call):
    tok = tkz.Tokenizer.from_json(json.dumps(CFG))
    assert call(tok, None) == INVALID
    tok.close()
    wide = tkz.Tokenizer.from_json(_wide_vocab_json())
    assert wide.info()["compact_tables"] == 0
    assert call(wide, ctypes.byref(tkz.pack_params(8, dtype=np.uint16))) == INVALID
    wide.close()


def test_truncation_or_padding_refused_on_the_host_entry_point():
    p = tkz.pack_params(8)
    tok = tkz.Tokenizer.from_json(json.dumps(CFG))
    tok.set_truncation(4)
    assert _host_call(tok, ctypes.byref(p)) == INVALID
    tok.set_truncation(None)
    tok.set_padding(6, pad_id=5)
    assert _host_call(tok, ctypes.byref(p)) == INVALID
    tok.close()


def test_python_encode_pack_raises_invalid_argument():
    tok = tkz.Tokenizer.from_json(json.dumps(CFG))
    off = np.array([0, 3], dtype=np.uint64)
    for kw in (dict(seq_len=0), dict(seq_len=8, bos_id=65536, dtype=np.uint16),
               dict(seq_len=8, eos_id=65536, dtype=np.uint16), dict(seq_len=8, pad_id=1 << 20, dtype=np.uint16)):
        with pytest.raises(tkz.TokenizerError) as e:
            tok.encode_pack(b"a b", off, **kw)
        assert e.value.code == INVALID, kw
    with pytest.raises(ValueError):
        tok.encode_pack(b"a b", off, 8, dtype=np.uint64)
    tok.set_padding(6, pad_id=5)
    with pytest.raises(tkz.TokenizerError) as e:
        tok.encode_pack(b"a b", off, 8)
    assert e.value.code == INVALID
    tok.close()
    wide = tkz.Tokenizer.from_json(_wide_vocab_json())
    with pytest.raises(tkz.TokenizerError) as e:
        wide.encode_pack(b"a b", off, 8, dtype=np.uint16)
    assert e.value.code == INVALID
    wide.close()
