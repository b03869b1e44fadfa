"""The memo-miss path of the word-level BPE: k_encode_blk's keyed short lists, k_bpe_short
and k_bpe_deferred with one-bucket merge probes.

Every case compares row_ptr, ids and offsets bit-exactly with the C++ oracle. The inputs
are small and sit where these kernels can go wrong:

- a short-list entry carries the word's normalized bytes (its memo key) and k_bpe_short
  never reads the input bytes, so the key must be right wherever the word lies: across a
  chunk end (the staged tail), ending exactly at a chunk end, at the end of a batch whose
  size is no multiple of 16 B, lowercased once (not twice), with multi-byte and invalid
  UTF-8;
- a chunk's list holds up to one entry per byte of the chunk (1-byte docs: every byte a
  word), at the smallest and the largest chunk size;
- the length-bucket queues run when 64 entries wait: batches that leave exactly 64 and 65;
- the overflow bitmap sends a probe to the second bucket only where some key overflowed:
  random compact tables filled to about one key per two-slot bucket, where a large share
  of the keys sits in its second bucket, memo on and off;
- the two-bucket code: a compact table's bitmap always fits LDS (< 65,535 merges: at most
  2^16 buckets, 8 KiB), so "too large" cannot occur there; the compact two-bucket
  instantiations are run with the bitmap switched off (TKZ_TWO_BUCKET=1). Ids past 2^16
  (the mid / wide tables) have no bitmap in the word-level kernels. A chain table
  (new_id == first) never takes k_encode_blk's lists: that routing is pinned too.
"""
import json
import os
import random

import numpy as np
import pytest

import tkz
from tkz import synth
from oracle import oracle as orc
from tests.test_segments import random_bpe_json

pytestmark = pytest.mark.gpu

NT = min(16, os.cpu_count() or 1)
WS = {"type": "Whitespace"}


def _pack(docs):
    off = np.zeros(len(docs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(d) for d in docs])
    data = np.frombuffer(b"".join(docs) + bytes(16), dtype=np.uint8).copy()
    return data, off


_ORACLES = {}


def _oracle(js):
    if js not in _ORACLES:
        _ORACLES[js] = orc.COracle(orc.RefTokenizer.from_json(js))
    return _ORACLES[js]


def _check(js, data, off, memo, max_ws=None, exp=None):
    tok = tkz.Tokenizer.from_json(js)
    tok.set_word_memo(memo)
    db = tkz.DeviceBatch(tok, data, off, max_workspace=max_ws)
    db.run()
    row, ids, offs = db.results()
    st = db.stats()
    db.free()
    tok.close()
    if exp is None:
        exp = _oracle(js).encode_batch(data, off, n_threads=NT)
    assert np.array_equal(row, exp[0])
    assert np.array_equal(ids, exp[1])
    assert np.array_equal(offs, exp[2])
    return st, exp


def _c1_words():
    """C1's words of 1..8 bytes, by length (from its own synthetic docs)."""
    data, off = synth.docs(1, 400)
    by_len = {n: [] for n in range(1, 9)}
    for w in bytes(data[: int(off[-1])]).split():
        if len(w) <= 8:
            by_len[len(w)].append(w)
    by_len[1] = [w[:1] for w in by_len[3][:200]]  # (the docs have no 1-byte words)
    assert all(len(v) >= 20 for v in by_len.values()), {k: len(v) for k, v in by_len.items()}
    return by_len


@pytest.fixture(scope="module")
def c1_words():
    return _c1_words()


def _short_docs(by_len, seed, n_docs, lo=1, hi=8):
    rng = random.Random(seed)
    docs = []
    for _ in range(n_docs):
        ws = [rng.choice(by_len[rng.randint(lo, hi)]) for _ in range(rng.randint(1, 24))]
        docs.append(b" ".join(ws))
    return docs


@pytest.mark.parametrize("cfg_id", [0, 1])
def test_every_word_a_short_miss(cfg_id, c1_words):
    """Memo off: every word of 1..8 B goes through the short list. 300 docs fill both
    length buckets with full and partial runs."""
    js = synth.tokenizer_json(cfg_id)
    data, off = _pack(_short_docs(c1_words, 11 + cfg_id, 300))
    st, _ = _check(js, data, off, memo=False)
    assert st["memo_hits"] == 0 and st["pretokens"] > 1000


@pytest.mark.parametrize("n_words", [64, 65])
@pytest.mark.parametrize("wlen", [3, 6])
def test_queue_of_exactly_64_and_65(n_words, wlen, c1_words):
    """One chunk (< 512 B) whose words all fall in one length bucket (<= 4 B: wlen 3;
    5..8 B: wlen 6): the queue holds exactly 64 entries (one full run, nothing left) or 65
    (a full run and a run of one)."""
    rng = random.Random(wlen * 100 + n_words)
    doc = b" ".join(rng.choice(c1_words[wlen]) for _ in range(n_words))
    assert len(doc) < 512
    data, off = _pack([doc])
    _check(synth.tokenizer_json(1), data, off, memo=False)


def _alpha_bytes(n, seed):
    rs = np.random.RandomState(seed)
    return np.frombuffer(b"etaoinshrdlu", np.uint8)[rs.randint(0, 12, size=n)]


@pytest.mark.parametrize("total", [512 * 6, 140 << 20], ids=["min_chunk", "max_chunk"])
def test_maximum_list_fill(total):
    """Chunks whose lists are as full as they can get, at the smallest chunk size (a tiny
    batch) and the largest (8 KiB: a batch of 140 MB, blank but for two chunks): 1-byte
    words separated by single spaces (one entry per two bytes), and 1-byte docs (every byte
    a word: one entry per byte, the bound the lists are laid out for)."""
    buf = np.full(total + 16, ord(" "), dtype=np.uint8)
    buf[total:] = 0
    ch = 8192 if total > (1 << 20) else 512
    a0 = 2 * ch                          # words + spaces: chunk 2 (and 3: the pattern runs on)
    buf[a0: a0 + 2 * ch: 2] = _alpha_bytes(ch, 1)
    b0 = 4 * ch                          # 1-byte docs: chunk 4
    buf[b0: b0 + ch] = _alpha_bytes(ch, 2)
    off = np.concatenate(([0], np.arange(b0, b0 + ch + 1), [total])).astype(np.uint64)
    st, _ = _check(synth.tokenizer_json(1), buf, off, memo=False)
    assert st["pretokens"] == 2 * ch


def test_key_provenance(c1_words):
    """Words of <= 8 B (and 9: the deferred side of the boundary) placed across a chunk end,
    ending exactly at one, and last in a batch whose size is no multiple of 16 B; chunk
    ends at every multiple of 512 B (a small batch), so every placement is made at several
    of them. Memo on and off (a miss's key is the one the memo probe used)."""
    rng = random.Random(5)
    js = synth.tokenizer_json(1)
    rare = [b"qzxjkvwy"[: n] for n in range(1, 9)] + [b"zqxjvkwyq"]  # no C1 vocab keys: misses
    for memo in (True, False):
        buf = bytearray(b" " * (512 * 40 + 7))
        for c in range(1, 40):
            end = 512 * c
            w = (rare if c % 2 else [rng.choice(c1_words[n]) for n in range(1, 9)] + [b"tokenizer"])[c % 9]
            shift = [0, 1, len(w) - 1, len(w) // 2][c % 4]  # ends at the chunk end, 1 past, starts 1 before, straddles
            s = end - len(w) + shift
            buf[s: s + len(w)] = w
        tail = rare[7]
        buf[len(buf) - len(tail):] = tail  # the batch's last word ends at its last byte
        assert len(buf) % 16 != 0
        cuts = sorted(rng.sample(range(1, len(buf)), 30))
        off = np.array([0] + cuts + [len(buf)], dtype=np.uint64)
        data = np.frombuffer(bytes(buf) + bytes(16), dtype=np.uint8).copy()
        _check(js, data, off, memo=memo)


def test_short_deferred_boundary(c1_words):
    """Words of exactly 8 and 9 bytes side by side: the last short-list length and the
    first deferred one."""
    rng = random.Random(9)
    w8 = c1_words[8]
    docs = []
    for _ in range(200):
        ws = []
        for _ in range(rng.randint(1, 12)):
            w = rng.choice(w8)
            ws.append(w if rng.random() < 0.5 else w + bytes([rng.choice(b"etaoin")]))
        docs.append(b" ".join(ws))
    data, off = _pack(docs)
    for memo in (True, False):
        _check(synth.tokenizer_json(1), data, off, memo=memo)


@pytest.mark.parametrize("memo", [True, False])
def test_lowercase_normalizer_keys(memo):
    """C2's Lowercase tokenizer: the key comes from the lowercased LDS stage and must not be
    lowercased again or left as typed. Mixed-case ASCII, 2..4-byte UTF-8 characters in words
    of <= 8 B, invalid lead bytes and a truncated sequence inside short words."""
    js = synth.tokenizer_json(2)
    assert json.loads(js)["normalizer"]["type"] == "Lowercase"
    d2, o2 = synth.docs(2, 60)
    base = [w for w in bytes(d2[: int(o2[-1])]).split() if len(w) <= 8][:400]
    rng = random.Random(2)
    mixed = [bytes(c ^ 0x20 if 97 <= c <= 122 and rng.random() < 0.5 else c for c in w) for w in base]
    utf = ["é", "Aé", "中b", "Aé中", "😀", "😀😀", "éé中", "Ωmega", "aé中z"]
    bad = [b"ab\xffcd", b"\x80abc", b"ab\xe4", b"\xf0\x9f\x98", b"A\xc3", b"Z\xfeZ"]
    words = mixed + [u.encode() for u in utf] * 8 + bad * 8
    assert all(len(w) <= 8 for w in words)
    rng.shuffle(words)
    docs = [b" ".join(words[i: i + 17]) for i in range(0, len(words), 17)]
    data, off = _pack(docs)
    _check(js, data, off, memo=memo)


@pytest.mark.parametrize("n_merges,alphabet", [(250, "abcdef"), (500, "abcdefgh"), (1900, "abcdefghij")])
def test_overflow_bitmap_random_tables(n_merges, alphabet):
    """Random compact merge tables of a few hundred to a few thousand merges, just under a
    power of two: about one key per two-slot bucket, so many first buckets are full and
    their later keys sit in the second bucket (the bitmap's set bits). Words over the same
    alphabet need exactly those merges. Memo on and off give the same (the oracle's) result."""
    js = random_bpe_json(100 + n_merges, alphabet=alphabet, n_merges=n_merges, pretok=WS, max_len=8)
    assert len(json.loads(js)["model"]["merges"]) > 0.9 * n_merges
    rng = random.Random(n_merges)
    docs = []
    for _ in range(250):
        ws = ["".join(rng.choice(alphabet) for _ in range(rng.randint(1, 16))) for _ in range(rng.randint(1, 20))]
        docs.append(" ".join(ws).encode())
    data, off = _pack(docs)
    _, exp = _check(js, data, off, memo=False)
    _check(js, data, off, memo=True, exp=exp)


@pytest.mark.parametrize("n_merges,alphabet", [(500, "abcdefgh")])
def test_compact_two_bucket_fallback(n_merges, alphabet, monkeypatch, c1_words):
    """The bitmap switched off at run time (TKZ_TWO_BUCKET=1, read at every launch): the
    compact two-bucket instantiations of k_bpe_short and k_bpe_deferred, which a compact
    table without a bitmap would take. The same random table and docs as above (words of
    1..16 B: both kernels), and C1's short words; memo off, then on."""
    monkeypatch.setenv("TKZ_TWO_BUCKET", "1")
    js = random_bpe_json(100 + n_merges, alphabet=alphabet, n_merges=n_merges, pretok=WS, max_len=8)
    rng = random.Random(n_merges)
    docs = []
    for _ in range(250):
        ws = ["".join(rng.choice(alphabet) for _ in range(rng.randint(1, 16))) for _ in range(rng.randint(1, 20))]
        docs.append(" ".join(ws).encode())
    data, off = _pack(docs)
    _, exp = _check(js, data, off, memo=False)
    _check(js, data, off, memo=True, exp=exp)
    data, off = _pack(_short_docs(c1_words, 41, 200))
    _check(synth.tokenizer_json(1), data, off, memo=False)


@pytest.mark.parametrize("shift", [70_000, 1_100_000])
def test_two_bucket_tables_mid_and_wide(shift, c1_words):
    """C1's vocab with every id moved past 2^16: below 2^20 the mid table (packed tokens
    through the short list), past it the wide table. Neither has a bitmap in the word-level
    kernels: the two-bucket / wide probes."""
    j = json.loads(synth.tokenizer_json(1))
    j["model"]["vocab"] = {k: i + shift for k, i in j["model"]["vocab"].items()}
    data, off = _pack(_short_docs(c1_words, 21, 200))
    _check(json.dumps(j), data, off, memo=False)


def test_chain_table_short_words():
    """A merge with new_id == first. Such a table never reaches k_encode_blk's short lists
    (launch_main sends it to k_encode, whose own queues run the literal loop), so this runs
    none of the miss kernels: it pins that routing, with words of <= 8 B, against the oracle."""
    cfg = {"model": {"type": "BPE", "vocab": {"a": 0, "": 1, "b": 2, "ab": 3, "aa": 4, "bb": 5, "c": 6, "ca": 7},
                     "merges": ["a ", "b b", "a b", "a a", "c a"]},
           "pre_tokenizer": WS}
    rng = random.Random(3)
    docs = [b" ".join(bytes(rng.choice(b"abc") for _ in range(rng.randint(1, 9))) for _ in range(rng.randint(1, 30)))
            for _ in range(200)]
    data, off = _pack(docs)
    for memo in (True, False):
        _check(json.dumps(cfg), data, off, memo=memo)


def test_bounded_workspace_short_misses(c1_words):
    """The short lists live in the workspace: ~2.5 MB of short misses through a workspace
    for 1-MiB sub-batches (several passes over the same scratch)."""
    js = synth.tokenizer_json(1)
    tok = tkz.Tokenizer.from_json(js)
    ws = int(tkz.lib().tkz_device_workspace_size_sub(tok.handle, 1 << 20))
    tok.close()
    data, off = _pack(_short_docs(c1_words, 31, 40_000))
    assert int(off[-1]) > (2 << 20)
    st, _ = _check(js, data, off, memo=False, max_ws=ws)
    assert st["sub_batches"] >= 2, st
