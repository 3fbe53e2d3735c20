"""The cases of tests/test_gpu_sumproduct_identity.py and of tests/golden/make_sumproduct_parent.py, which recorded their expected outputs
(tests/golden/sumproduct_parent.npz) once, on the GPU, from the commit BEFORE the sum-product sweeps of post_kernel and
edits_fb_kernel were written once in csrc/lattice_sums.h.  The kernels built from the shared pieces must reproduce those outputs bit
for bit.  Inputs come from seeds; `tok` and the start windows come from wfl_align / wfl_align_windowed / wfl_align_min_duration, which
that change did not touch.

Every call is one ragged batch.  Shapes are the smallest at which a sweep can go wrong:
  configs   N in CONFIG_N, T = N + 12: the five (threads, slots) configurations and their boundaries, tokens with 1, 2 and 4
            alternatives and repeated tokens
  frames    N = 5 at T in FRAME_T (the renormalisation period of 16; the 128-frame blocks and checkpoints), T = 0 with and without
            tokens, and three clips of many alternatives / repeated tokens
  C12, C141, C1024   N = 5, T = 40: 32, 7 and 1 logits rows per stage
each through the four posterior entries (ENTRIES), with one more clip per call that ends in a status.  Start windows are +-2 frames
round the search's starts; minimum durations are drawn from {1, 2, 3, 8} as far as the clip's spare frames allow (all but two).
  edits / insertions   P in {0, 6, 70} substitutes, with and without windows, at (N, T) = (5, 17) and (128, 140); P = 6 at
            (2048, 2060); a substitute class out of range (status 4 for every clip)

The golden file stays under 256 KB: an output of more than FULL_BYTES bytes is kept as the SHA-256 of its bytes (pack)."""
import hashlib

import numpy as np
import torch

import posterior_ref as P
from wfl_asr_amd import align as AL

O_ID = 0
CONFIG_N = (0, 1, 5, 127, 128, 512, 1024, 2048)
FRAME_T = (5, 15, 16, 17, 127, 128, 129, 257)
STAGE_C = (12, 141, 1024)
ENTRIES = ("plain", "windowed", "mind", "mind_windowed")
FULL_BYTES = 16384


def pairs(C):
    return [(2 * p - 1, 2 * p) for p in range(1, (C - 1) // 2 + 1)]


def clip(T, N, C, seed, n_alt=1, repeat=False, boost=4.0):
    """-> dict(z [T, C] float32, alts, gaps, D): D the minimum durations the entries with them use."""
    rng = np.random.default_rng(seed)
    ph = pairs(C)
    alts = []
    for k in range(N):
        if repeat and k % 3 == 1:
            alts.append(alts[-1])                         # the same token twice in a row
            continue
        alts.append([ph[int(j)] for j in rng.choice(len(ph), size=n_alt, replace=False)])
    z = P.planted_logits(T, N, C, alts, [O_ID], rng, boost)
    D, spare = [1] * N, T - N - 2
    for k in rng.permutation(N):
        d = int(rng.choice((1, 2, 3, 8)))
        if d - 1 <= spare:
            D[int(k)], spare = d, spare - (d - 1)
    return dict(z=z, alts=alts, gaps=[O_ID], D=D)


def config_clips(C=31):
    return [clip(N + 12, N, C, 1000 + N, n_alt=(1, 2, 4)[i % 3], repeat=i % 2 == 1, boost=4.0 * (i % 2)) for i, N in enumerate(CONFIG_N)]


def frame_clips(C=31):
    out = [clip(T, 5, C, 2000 + T, boost=4.0 * (i % 2)) for i, T in enumerate(FRAME_T)]
    out += [clip(0, 5, C, 2001), clip(0, 0, C, 2002)]
    return out + [clip(60, 20, C, 2003, n_alt=4), clip(60, 20, C, 2004, n_alt=2, repeat=True), clip(50, 12, C, 2005, repeat=True, boost=0.0)]


def stage_clips(C):
    return [clip(40, 5, C, 3000 + C, n_alt=2, boost=0.0), clip(40, 5, C, 3001 + C, boost=4.0)]


def status_clip(entry, C):
    """The clip an entry's call ends with, and the status it must come back with: a tok with a token removed (8), N over the cap (2),
    a D_k of 9 (4), windows no path meets (1: reported where there are durations; without them such a clip's tok is no path, 8)."""
    if entry == "plain":
        return clip(30, 4, C, 4001), 8
    if entry == "windowed":
        return clip(1, AL.MAX_TOKENS + 1, C, 4002, boost=0.0), 2
    if entry == "mind":
        c = clip(77, 5, C, 4003)
        c["D"] = [2, 3, 9, 1, 1]
        return c, 4
    c = clip(30, 4, C, 4004)
    c["windows"] = [(5, 4)] * 4                              # lo > hi: never
    return c, 1


def _upload(clips):
    T = [len(c["z"]) for c in clips]
    offs = np.concatenate([[0], np.cumsum(T)[:-1]]).astype(np.int64)
    lg = torch.from_numpy(np.ascontiguousarray(np.concatenate([c["z"] for c in clips]))).cuda()
    return (lg, T, [c["alts"] for c in clips], [c["gaps"] for c in clips]), offs


def _windows(clips, tok, status, offs):
    """+-2 frames round the first frame of every token in `tok`; a clip the search gave a status keeps its own (or open) windows."""
    tok = tok.cpu().numpy()
    wins = []
    for c, o, st in zip(clips, offs, status.cpu().numpy()):
        T, N = len(c["z"]), len(c["alts"])
        if st != 0 or "windows" in c:
            wins.append(c.get("windows"))
            continue
        t = tok[o:o + T]
        first = [int(np.nonzero(t == k)[0][0]) for k in range(N)]
        wins.append([(max(s - 2, 0), min(s + 2, T - 1)) for s in first])
    return wins


def _packed(clips, windowed, mind):
    """-> (args, offs, the PackedClips of the entry, its search's tok)"""
    args, offs = _upload(clips)
    mins = [c["D"] for c in clips] if mind else None
    packed = AL.pack_clips(*args, offs, min_frames=mins)
    _, tok, _, st = AL.viterbi_align(*args, O_ID, packed=packed)
    if windowed:
        packed = AL.pack_clips(*args, offs, windows=_windows(clips, tok, st, offs), min_frames=mins)
        _, tok, _, st = AL.viterbi_align(*args, O_ID, packed=packed)
    return args, offs, packed, tok


def run_posterior(clips, entry, C):
    extra, code = status_clip(entry, C)
    clips = clips + [extra]
    mind = entry.startswith("mind")
    args, offs, packed, tok = _packed(clips, entry.endswith("windowed"), mind)
    if entry == "plain":                                     # token 1 of the last clip leaves its tok
        t = tok[int(offs[-1]):]
        t[t == 1] = -1
    logz, tp, mu, sd, st = (AL.duration_posteriors if mind else AL.alignment_posteriors)(*args, O_ID, tok, packed=packed)
    torch.cuda.synchronize()
    out = dict(logz=logz, tok_post=tp, start_mean=mu, start_sd=sd, status=st)
    out = {k: v.cpu().numpy() for k, v in out.items()}
    assert int(out["status"][-1]) == code, (entry, out["status"])
    return out


def edit_clips(C=141):
    return [clip(17, 5, C, 5001, n_alt=2), clip(140, 128, C, 5002, repeat=True)]


def run_edits(clips, subs, windowed, ins):
    args, offs, packed, _ = _packed(clips, windowed, False)
    logz, out, st = (AL.insertion_scores if ins else AL.edit_scores)(*args, O_ID, subs, frame_offsets=offs, packed=packed)
    torch.cuda.synchronize()
    return dict(logz=logz.cpu().numpy(), scores=out.cpu().numpy(), status=st.cpu().numpy())


def pack(outputs):
    """name -> array as the golden file keeps it: the array itself, or (above FULL_BYTES) the SHA-256 of its bytes."""
    out = {}
    for k, v in outputs.items():
        v = np.ascontiguousarray(v)
        if v.nbytes > FULL_BYTES:
            out[k + ".sha256"] = np.frombuffer(hashlib.sha256(v.tobytes()).digest(), np.uint8).copy()
        else:
            out[k] = v
    return out


def run_all():
    """-> {call.entry.output: array}, packed.  Every call of every case, in a fixed order."""
    res = {}
    calls = [("configs", config_clips(), 31), ("frames", frame_clips(), 31)] + [(f"C{C}", stage_clips(C), C) for C in STAGE_C]
    for name, clips, C in calls:
        for entry in ENTRIES:
            for k, v in run_posterior(clips, entry, C).items():
                res[f"{name}.{entry}.{k}"] = v
    for ins in (False, True):
        what = "insertions" if ins else "edits"
        for P_ in (0, 6, 70):
            for windowed in (False, True):
                for k, v in run_edits(edit_clips(), pairs(141)[:P_], windowed, ins).items():
                    res[f"{what}.P{P_}.{'windowed' if windowed else 'open'}.{k}"] = v
        for k, v in run_edits([clip(2060, 2048, 31, 5003)], pairs(31)[:6], False, ins).items():
            res[f"{what}.N2048.{k}"] = v
        bad = run_edits([clip(20, 3, 31, 5004), clip(30, 5, 31, 5005)], pairs(31)[:2] + [(31, 2)], False, ins)
        assert list(bad["status"]) == [4, 4]
        for k, v in bad.items():
            res[f"{what}.bad_substitute.{k}"] = v
    return pack(res)
