"""The cases of tests/test_gpu_epilogue_identity.py and of tests/golden/make_epilogue_parent.py, which recorded their expected
outputs (tests/golden/epilogue_parent.npz) once, on the GPU, from the commit BEFORE the epilogue / attention / LayerNorm kernels were
trimmed of the vector-ALU work their results do not need.  The trimmed kernels must reproduce those outputs bit for bit.

Model: the synthetic Whisper-tiny encoder (d = 384, 1500 frames per 30 s clip) behind the 2-Conformer head, default precision.
  b6      six clips: 9 000 rows; fc1 (N = 1536) is 6 column tiles x 47 row tiles = 282 tiles for 256 persistent workgroups, so
          workgroups cross a tile boundary and run the streaming GEMM's in-loop epilogue
  b1      one clip: every launch is at most one tile per workgroup -- only the final epilogue runs
  ragged  three clips of different lengths (`lens`)"""
import numpy as np
import torch

import synthetic as synth
from wfl_asr_amd.tagger import BIOPhonemeTagger

SEED = 83
L = 480000                       # 30 s at 16 kHz
CLIP0 = 4100
THRESHOLD = 0.5
CASES = {
    "b6": dict(B=6, lens=None),
    "b1": dict(B=1, lens=None),
    "ragged": dict(B=3, lens=np.array([480000, 301234, 170000], np.int32)),
}


def config():
    return synth.base_config("whisper", whisper_model="openai/whisper-tiny", enable_bilstm=False, enable_dilated_conv=False)


def build_model():
    cfg = config()
    labels = synth.make_labels(70)
    sd = synth.make_state_dict(cfg, len(labels), seed=SEED)
    m = BIOPhonemeTagger(cfg, labels)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m.to("cuda").eval()
    return m


def clips(n):
    return synth.make_batch(CLIP0, n, L, seed=SEED)


def run_case(m, wav6, name):
    """-> dict of the four TagBatch arrays as integers (floats as their bit patterns)."""
    c = CASES[name]
    B, lens = c["B"], c["lens"]
    wav = wav6[:B].copy()
    if lens is not None:
        for i in range(B):
            wav[i, int(lens[i]):] = 0.0
    lang = (np.arange(B) % 2).astype(np.int64)
    out = m.label(torch.from_numpy(wav).cuda(), lang, threshold=THRESHOLD, lens=lens)
    torch.cuda.synchronize()
    m.check(B, L)
    return {
        "ids": out.ids.cpu().numpy().astype(np.int16),
        "argmax": out.argmax.cpu().numpy().astype(np.int16),
        "maxprob": out.maxprob.cpu().numpy().astype(np.float32).view(np.uint32),
        "offsets": out.offsets.cpu().numpy().astype(np.float32).view(np.uint32),
    }
