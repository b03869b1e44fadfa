"""Throughput of sequence packing on C1 (1M x 512-B docs, 32k BPE), one MI355X.

Device: tkz_pack_batch_device on the encode CSR resident in HBM (seq_len 2048, EOS
separators), u32 and u16 ids, with and without segment + position ids, beside
tkz_pad_batch_device (truncate + pad to [n, 128]) on the same CSR in the same process.
Host: tkz_encode_pack_batch (u16, ids only) against tkz_encode_batch, same tokenizer, same
page-locked input. Every variant is warmed up, then timed in ROUNDS alternating series of K
calls (host clock around calls that end in a stream synchronise); medians and ranges over
the rounds. usage: tools/bench_pack.py [--docs N] [--out FILE.json] [--no-host]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tokenizer-zig_amd")]
import tkz  # noqa: E402
from tkz import synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=1_000_000)
ap.add_argument("--out", default=None)
ap.add_argument("--no-host", action="store_true", help="device rows only (a short run for a kernel trace)")
args = ap.parse_args()

K, ROUNDS, HOST_ROUNDS = 50, 7, 5
SEQ, EOS, PAD_LEN = 2048, 2, 128
PEAK = 8.0e12  # HBM3E, bytes/s (spec)
L = tkz.lib()
if not tkz.device_available():
    raise SystemExit("bench_pack: no GPU visible to libtkz")
tok = tkz.Tokenizer.from_json(synth.tokenizer_json(1))
data, off = synth.docs(1, args.docs)
db = tkz.DeviceBatch(tok, data, off)
db.run()
db.sync()
n = db.n_docs
T = db.n_tokens()


def series(fns, rounds, k):
    """fns: name -> callable queuing one call. Alternating series; per-call seconds per round."""
    for fn in fns.values():
        fn()
    L.tkz_synchronize(tok.handle)
    times = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            t0 = time.perf_counter()
            for _ in range(k):
                fn()
            L.tkz_synchronize(tok.handle)
            times[name].append((time.perf_counter() - t0) / k)
    return times


def summary(ts):
    return {"ms_median": round(statistics.median(ts) * 1e3, 4), "ms_min": round(min(ts) * 1e3, 4),
            "ms_max": round(max(ts) * 1e3, 4)}


# ---- device: pack variants and pad on the same CSR ----
fns, traffic = {}, {}
keep = []
for width, dtype in ((4, np.uint32), (2, np.uint16)):
    for opt in (False, True):
        p = tkz.pack_params(SEQ, None, EOS, 0, dtype)
        rows = int(L.tkz_pack_rows(ctypes.byref(p), n, T))
        n_pos = rows * SEQ
        out = tkz.DeviceBuffer(n_pos * width + 16)
        seg = tkz.DeviceBuffer(n_pos * 4 + 16) if opt else None
        pos = tkz.DeviceBuffer(n_pos * 4 + 16) if opt else None
        cnt, st = tkz.DeviceBuffer(16), tkz.DeviceBuffer(16)
        st.zero()
        keep += [out, seg, pos, cnt, st, p]

        def call(p=p, rows=rows, out=out, seg=seg, pos=pos, cnt=cnt, st=st):
            rc = L.tkz_pack_batch_device(tok.handle, db.d_row.ptr, db.d_ids.ptr, n, ctypes.byref(p), rows, out.ptr,
                                         seg.ptr if seg else None, pos.ptr if pos else None, None, cnt.ptr, st.ptr,
                                         None)
            if rc:
                raise RuntimeError(rc)
        name = f"pack u{8 * width}" + (" + segment + position ids" if opt else "")
        fns[name] = call
        traffic[name] = {"read": T * 4 + (n + 1) * 8, "written": n_pos * width + (2 * n_pos * 4 if opt else 0),
                         "status": st, "rows": rows}

tok.set_truncation(PAD_LEN)
tok.set_padding(PAD_LEN)
cap = int(L.tkz_pad_capacity(tok.handle, n, T))
wsb = int(L.tkz_pad_workspace_size(n))
pbufs = [tkz.DeviceBuffer(x) for x in ((n + 1) * 8, cap * 4, cap * 8, cap * 4, cap * 4, cap * 4, wsb)]


def pad():
    rc = L.tkz_pad_batch_device(tok.handle, db.d_row.ptr, db.d_ids.ptr, db.d_offs.ptr, n, *[b.ptr for b in pbufs[:6]],
                                pbufs[6].ptr, wsb, None)
    if rc:
        raise RuntimeError(rc)


fns["pad to [n, 128] (tkz_pad_batch_device)"] = pad
traffic["pad to [n, 128] (tkz_pad_batch_device)"] = {
    "read": (n + 1) * 8 + min(T, n * PAD_LEN) * 12, "written": n * PAD_LEN * (4 + 8 + 4 * 3) + (n + 1) * 8}
times = series(fns, ROUNDS, K)
result = {"config": "C1", "docs": n, "input_bytes": db.total, "tokens": T, "seq_len": SEQ, "separators": "eos",
          "calls_per_series": K, "series": ROUNDS, "device": [], "host": []}
for name, ts in times.items():
    tr = traffic[name]
    if "status" in tr:
        s = np.zeros(4, dtype=np.uint32)
        tr["status"].download(s)
        if s[0]:
            raise SystemExit(f"bench_pack: {name} reported status {s[0]}")
    med = statistics.median(ts)
    row = {"row": name, **summary(ts), "bytes_read": tr["read"], "bytes_written": tr["written"],
           "written_GB_per_s": round(tr["written"] / med / 1e9, 1),
           "read_plus_written_GB_per_s": round((tr["read"] + tr["written"]) / med / 1e9, 1),
           "read_plus_written_GB_per_s_range": [round((tr["read"] + tr["written"]) / t / 1e9, 1)
                                                for t in (max(ts), min(ts))],
           "fraction_of_8TBps": round((tr["read"] + tr["written"]) / med / PEAK, 3)}
    result["device"].append(row)
    print(json.dumps(row), flush=True)
tok.set_truncation(None)
tok.set_padding(None, enabled=False)
for b in pbufs + [x for x in keep if isinstance(x, tkz.DeviceBuffer)]:
    b.free()
db.free()

if args.no_host:
    raise SystemExit(0)

# ---- host: packed u16 rows against the CSR, same page-locked input ----
pin = tkz.HostBuffer(len(data))
pin.array[:] = data
off = np.ascontiguousarray(off, dtype=np.uint64)
dp = pin.array.ctypes.data_as(ctypes.c_void_p)
op = off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
p16 = tkz.pack_params(SEQ, None, EOS, 0, np.uint16)
out_bytes = {}


def host_csr():
    b = tkz._Batch()
    rc = L.tkz_encode_batch(tok.handle, dp, op, n, ctypes.byref(b))
    if rc:
        raise RuntimeError(rc)
    out_bytes["tkz_encode_batch (CSR)"] = (n + 1) * 8 + int(b.n_tokens) * 12
    L.tkz_batch_free(ctypes.byref(b))


def host_pack():
    b = tkz._Packed()
    rc = L.tkz_encode_pack_batch(tok.handle, dp, op, n, ctypes.byref(p16), ctypes.byref(b))
    if rc:
        raise RuntimeError(rc)
    out_bytes["tkz_encode_pack_batch (u16 ids only)"] = int(b.n_rows) * SEQ * 2
    L.tkz_packed_free(ctypes.byref(b))


hf = {"tkz_encode_batch (CSR)": host_csr, "tkz_encode_pack_batch (u16 ids only)": host_pack}
for fn in hf.values():  # (the first CSR batch of a tokenizer sizes its chunk pipeline)
    fn()
times = series(hf, HOST_ROUNDS, 2)
for name, ts in times.items():
    med = statistics.median(ts)
    row = {"row": name, **summary(ts), "output_bytes": out_bytes[name],
           "input_GB_per_s": round(db.total / med / 1e9, 2),
           "input_GB_per_s_range": [round(db.total / t / 1e9, 2) for t in (max(ts), min(ts))]}
    result["host"].append(row)
    print(json.dumps(row), flush=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
