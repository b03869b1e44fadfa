#!/usr/bin/env python3
"""Overflow share of the cuckoo merge tables of the bench configs: builds
tools/over_share.cpp and feeds it each config's accepted merges (tokenizer.cpp's rules).
usage: python tools/over_share.py [cfg ...]   (default 1 5 7)"""
import json
import os
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tokenizer-zig_amd"))
from tkz import synth  # noqa: E402

tmp = tempfile.TemporaryDirectory()  # (removed at exit)
exe = os.path.join(tmp.name, "over_share")
subprocess.run(["g++", "-O2", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                os.path.join(REPO, "tools", "over_share.cpp"), "-o", exe], check=True)
for cfg in [int(a) for a in sys.argv[1:]] or [1, 5, 7]:
    m = json.loads(synth.tokenizer_json(cfg))["model"]
    vocab = {k.encode(): v for k, v in m["vocab"].items()}
    lines, rank = [], 0
    for it in m.get("merges", []):
        if isinstance(it, str):
            parts = it.encode().split(b" ")
            if len(parts) < 2:
                continue
            a, b = parts[0], parts[1]
        else:
            a, b = it[0].encode(), it[1].encode()
        if a not in vocab or b not in vocab or len(a) + len(b) > 512 or a + b not in vocab:
            continue
        lines.append(f"{vocab[a]} {vocab[b]} {rank} {vocab[a + b]}")
        rank += 1
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
    print(f"C{cfg}: {out.strip()}")
