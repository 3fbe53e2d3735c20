"""-m gpu: the workspace plan of csrc/model.hip (Plan::bufs, make_plan).

A. The layout: wfl_workspace_bytes / wfl_head_workspace_bytes of a set of tiny models equal the sizes recorded from the commit
   named in tests/golden/workspace_bytes.json (every offset of the plan is a partial sum of the same take() sizes, so the total moves
   when any of them does).  No kernel is launched.
B. The forward does not see the workspace's history: labelling on a workspace whose every byte was overwritten gives, bit for bit,
   what labelling on the freshly zeroed one gave -- the invariant begin_forward and zero_shared_buffers exist for.
   BiLSTM heads are left out of B: the recurrence's exchange area is protocol state of its own (csrc/lstm.hip).

`python tests/test_gpu_workspace_plan.py COMMIT` (with the package of that commit first on PYTHONPATH) writes the golden file."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import synthetic as synth
from cases import tiny_whisper_config, tiny_wavlm_config
from wfl_asr_amd.tagger import BIOPhonemeTagger

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "workspace_bytes.json")


def _whisper(**kw):
    return tiny_whisper_config(enable_bilstm=False, **kw)


def _whisper_fp8():
    cfg = _whisper(weight_dtype="fp8")
    cfg["model"]["encoder_arch"] = dict(d_model=256, layers=2, heads=4, ffn=256, n_mels=80, max_positions=100)   # fp8: multiples of 256
    return cfg


CONFIGS = {
    "whisper_tiny": _whisper,
    "whisper_tiny_fp8": _whisper_fp8,
    "wavlm_tiny_group": lambda: tiny_wavlm_config(False, enable_bilstm=False),
    "wavlm_tiny_stable": lambda: tiny_wavlm_config(True, enable_bilstm=False),
    "none": lambda: synth.base_config("none", enable_bilstm=False),
    "whisper_tiny_padded_heads": lambda: _whisper(conformer_heads=4),       # head size 16 runs as 32: conf_da = 128 != d_model = 64
    "whisper_tiny_bilstm": lambda: tiny_whisper_config(enable_bilstm=True),
}
BATCHES = (1, 3)
LENGTHS = (16000, 12347)            # 12347: no multiple of a mel hop (160, 320) or of the WavLM strides (5, 2)
HEAD_FRAMES = 37


def _config(name, precision):
    cfg = CONFIGS[name]()
    cfg["model"]["precision"] = precision
    return cfg


def _cases():
    for name in CONFIGS:
        for precision in ("default", "high"):
            if precision == "high" and name == "whisper_tiny_fp8":
                continue                                                    # (the model refuses fp8 weights at precision high)
            yield name, precision


def _measure():
    """{case: {"B,L": wfl_workspace_bytes, "head B,T": wfl_head_workspace_bytes}}: handles only, nothing is uploaded or launched"""
    labels = synth.make_labels(5)
    sizes = {}
    for name, precision in _cases():
        m = BIOPhonemeTagger(_config(name, precision), labels)
        row = {}
        for B in BATCHES:
            for L in LENGTHS:
                row[f"{B},{L}"] = int(m._lib.wfl_workspace_bytes(m._handle, B, L))
            row[f"head {B},{HEAD_FRAMES}"] = int(m._lib.wfl_head_workspace_bytes(m._handle, B, HEAD_FRAMES))
        sizes[f"{name}/{precision}"] = row
    return sizes


def test_workspace_sizes_are_the_recorded_ones():
    with open(GOLDEN) as f:
        want = json.load(f)["sizes"]
    got = _measure()
    assert sorted(got) == sorted(want)
    for case in want:
        assert got[case] == want[case], case
    assert all(v > 0 for row in got.values() for v in row.values())


RAGGED = np.array([16000, 9000, 4000], np.int32)
HISTORY_CASES = [("whisper_tiny", None), ("wavlm_tiny_group", RAGGED), ("none", RAGGED), ("whisper_tiny_padded_heads", None)]


@pytest.mark.parametrize("precision", ["default", "high"])
@pytest.mark.parametrize("name,lens", HISTORY_CASES, ids=[c[0] for c in HISTORY_CASES])
def test_forward_does_not_see_the_workspace_history(name, lens, precision):
    cfg = _config(name, precision)
    labels = synth.make_labels(5)
    sd = synth.make_state_dict(cfg, len(labels), seed=91)
    m = BIOPhonemeTagger(cfg, labels)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m.to("cuda").eval()
    B, L = 3, 16000
    wav = synth.make_batch(930, B, L, seed=91)
    if lens is not None:
        for i, n in enumerate(lens):
            wav[i, n:] = 0.0
    x = torch.from_numpy(wav).cuda()
    lang = np.array([0, 1, 0], np.int64)

    def run():
        out = m.label(x, lang, threshold=0.4, lens=lens, want_logits=True)
        m.check(B, L)                                                       # synchronises; raises on a device-side error word
        return out

    fresh = run()                                                           # the workspace as allocated: zeros
    assert m._ws is not None and m._ws.dtype == torch.uint8
    # 0x3C in every byte: finite and small as bf16 (0x3C3C), as fp32 and as fp64, so a stale value times a zero-padded weight is still 0
    m._ws.fill_(0x3C)
    stale = run()
    for field in ("ids", "argmax", "maxprob", "offsets", "logits"):
        assert torch.equal(getattr(fresh, field), getattr(stale, field)), field
    assert int(fresh.status.item()) == 0 and int(stale.status.item()) == 0


if __name__ == "__main__":
    with open(GOLDEN, "w") as f:
        json.dump({"note": "wfl_workspace_bytes(B, L) and wfl_head_workspace_bytes(B, T) of tests/test_gpu_workspace_plan.py's tiny "
                           "models, recorded from a build of commit " + sys.argv[1],
                   "sizes": _measure()}, f, indent=1, sort_keys=True)
        f.write("\n")
