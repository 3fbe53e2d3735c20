#!/usr/bin/env python3
"""Diagnostic (not product): time wfl_op_attention at the Conformer head sizes.  usage: attn_bench.py d heads B [T] [--waves 4,8,12] [--rounds N]
(run once per WFL_ATTN_VARIANT value to A/B the head_dim 64 / 384 kernels; --waves times the head_dim 256 forms that WFL_ATTN_WAVES selects
side by side in ONE process, interleaved round by round -- the library reads the variable at every launch -- and checks that their outputs
are bit-identical)"""
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import wfl_asr_amd  # noqa: F401,E402
from wfl_asr_amd import _lib  # noqa: E402

argv = sys.argv[1:]


def _opt(name, default):
    if name in argv:
        i = argv.index(name)
        v = argv[i + 1]
        del argv[i:i + 2]
        return v
    return default


waves = _opt("--waves", None)
rounds = int(_opt("--rounds", "5"))
d, heads, B = int(argv[0]), int(argv[1]), int(argv[2])
T = int(argv[3]) if len(argv) > 3 else 1500
P, lead = T + 20, 16
R = lead + B * P + 256
lib = _lib.load()
qkv = (torch.randn(R, 3 * d, device="cuda") * 0.5).to(torch.bfloat16)
o = torch.zeros(R, d, dtype=torch.bfloat16, device="cuda")
p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
s = C.c_void_p(torch.cuda.current_stream().cuda_stream)


def run():
    _lib.check(lib.wfl_op_attention(p(qkv), 3 * d, lead, p(qkv, 2 * d * 2), 3 * d, p(o), d, B, T, P, heads, d, s), "attn")


def timed(n=10):
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


fl = 4.0 * B * T * T * d
head = f"d {d} heads {heads} (head_dim {d // heads}) B {B} T {T}"
if waves is None:
    ms = timed()
    print(f"{head} variant {os.environ.get('WFL_ATTN_VARIANT', '0')}: {ms * 1e3:.1f} us, {fl / ms / 1e9:.0f} TFLOP/s")
else:
    forms = waves.split(",")
    us = {w: [] for w in forms}
    outs = {}
    for r in range(rounds):
        for w in forms:
            os.environ["WFL_ATTN_WAVES"] = w
            us[w].append(timed() * 1e3)
            if r == 0:
                outs[w] = o.clone()
                o.zero_()
    for w in forms:
        t = sorted(us[w])
        same = torch.equal(outs[w], outs[forms[0]])
        print(f"{head} waves {w}: median {t[len(t) // 2]:.1f} us (min {t[0]:.1f}, max {t[-1]:.1f}; {rounds} rounds of 10 launches), "
              f"{fl / t[len(t) // 2] / 1e6:.0f} TFLOP/s, output {'identical to' if same else 'DIFFERS from'} waves {forms[0]}")
