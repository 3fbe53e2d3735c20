"""The scenario of tests/golden/label_viterbi_parent.json (recorded by tests/golden/make_label_viterbi_parent.py, held by
tests/test_gpu_label_viterbi_identity.py): one folder of six small files on the tiny Whisper checkpoint of test_gpu_align_e2e._setup
(no BiLSTM, max_positions 1500, seed 41), run through infer_folder once per option set of RUNS; every file the run writes and what it
prints are the record.  The six files fill one wave, so every run is one ragged batch in which clips leave at every stage:

  a.wav        7 s = 350 frames, a transcript of 91 tokens (SP spelled): aligned in every run; under min_duration 0.08 (4 frames, 364
               in all) no path, so it is searched, and scored, without its durations
  b.wav        4 s = 200 frames, 60 tokens: under min_duration 0.08 (4 frames) no path; its draft puts four starts on one frame, so
               under tolerance 0.02 (one frame either side) no path opens every token inside its window either
  long.wav     65 s, the hand-made draft of 64 tokens of test_gpu_align_min_duration_e2e.py (the token at 29.5 s moved to 29.94 s: with
               four frames at least its run crosses the seam at 30 s), the same labels as its transcript
  over.wav     3 s = 150 frames, 200 tokens: the search's status 1, the clip leaves the batch after the search
  unknown.wav  3 s, a transcript with a token the label set lacks: never in the batch
  zplain.wav   3 s, no transcript

EDITS_LIMIT: AL.EDITS_WORKSPACE_LIMIT of the `edits_insertions` run, 512 KiB.  The workspaces of a.wav, b.wav and long.wav (350, 200
and 3250 frames) are 545 536, 158 720 and 2 561 792 bytes for edit_scores and 366 336, 107 520 and 3 394 048 for insertion_scores:
edit_groups yields three groups for the edits, [a], [b], [long], and two for the insertions, [a, b], [long], so every scoring call runs
on a sub-batch packed again from the clips the search aligned.

The last run, `kernel_fallback`, is `durations_scores_draft` with AL.windows_feasible replaced by `lambda *a: True`: the host rule
finds nothing, a.wav, b.wav and over.wav come back from the search with status 1, b.wav twice, and the fallback loop runs both rounds
(durations dropped, then windows dropped)."""
import contextlib
import io
import os

import numpy as np
import torch
import yaml

import synthetic as synth
from cases import tiny_whisper_config

LABELS = sorted(["O"] + [f"{t}-{p}" for p in ("p00", "p01", "p02", "p03", "SP", "AP") for t in ("B", "I")])
CT = 0.3
EDITS_LIMIT = 1 << 19
SEED = 41

RUNS = {
    "plain": {},
    "scores": dict(align_scores=True),
    "draft_scores": dict(align_draft=True, draft_tolerance=0.02, align_scores=True),
    "edits_insertions": dict(align_edits=True, align_insertions=True),
    "durations": dict(min_duration=0.08),
    "durations_scores_draft": dict(min_duration=0.08, duration_scores=True, align_draft=True, draft_tolerance=0.02),
    "kernel_fallback": dict(min_duration=0.08, duration_scores=True, align_draft=True, draft_tolerance=0.02),
}


def transcript(n, seed=7):
    """test_gpu_align_min_duration_e2e._transcript: n random tokens with SP spelled in the middle."""
    names = [str(x) for x in np.random.default_rng(seed).choice(["p00", "p01", "p02", "p03"], size=n)]
    return names[:n // 2] + ["SP"] + names[n // 2:]


def long_draft():
    names = ["p00", "p01", "p02", "p03"]
    return [((29.94 if k == 29 else 0.5 + k), 0.9 + k, names[k % 4] if k != 40 else "SP") for k in range(64)]


def b_draft():
    """A token every 0.06 s from 0.1 s; tokens 10 .. 13 open at one time."""
    return [(0.1 + 0.06 * (10 if 10 <= k <= 13 else k), 0.1 + 0.06 * (k + 1), t) for k, t in enumerate(transcript(59))]


def build(d):
    """The checkpoint, its config, the folder `wavs` and the drafts under the directory `d` (a str)."""
    from wfl_asr_amd import audio as A
    from wfl_asr_amd import native_post as npost
    cfg = tiny_whisper_config(enable_bilstm=False)
    cfg["model"]["encoder_arch"]["max_positions"] = 1500
    cfg["output"]["save_dir"] = os.path.join(d, "save")
    cfg["postprocess"] = {"median_filter": 3, "merge_segments": "right", "confidence_threshold": CT}
    for sub in ("save", "wavs", "drafts"):
        os.makedirs(os.path.join(d, sub))
    with open(os.path.join(d, "save", "phonemes.txt"), "w") as f:
        f.write("\n".join(LABELS) + "\n")
    with open(os.path.join(d, "config.yaml"), "w") as f:
        yaml.safe_dump(cfg, f)
    torch.save({k: torch.from_numpy(v) for k, v in synth.make_state_dict(cfg, len(LABELS), seed=SEED).items()},
               os.path.join(d, "best_model.pt"))
    files = {"a": (800, 7, 0.9, transcript(90)), "b": (802, 4, 0.7, transcript(59)),
             "long": (801, 65, 0.8, [s[2] for s in long_draft()]), "over": (803, 3, 0.8, ["p00"] * 200),
             "unknown": (804, 3, 0.8, ["p00", "zz", "p01"]), "zplain": (805, 3, 0.8, None)}
    for name, (clip, sec, gain, tr) in files.items():
        A.write_wav(os.path.join(d, "wavs", name + ".wav"), synth.make_clip(clip, 16000 * sec, seed=SEED) * gain, 16000)
        if tr is not None:
            with open(os.path.join(d, "wavs", name + ".txt"), "w") as f:
                f.write(" ".join(tr))
    for name, draft in (("long", long_draft()), ("b", b_draft())):
        with open(os.path.join(d, "drafts", name + ".lab"), "wb") as f:
            f.write(npost.format_lab_tuples(draft))


def run(d, name):
    """One run of RUNS over the folder of build(d) -> {"stdout": what it printed, "files": {name: text of every file it wrote}}, the
    directory `d` spelled <TMP> in both."""
    from wfl_asr_amd import align as AL
    from wfl_asr_amd import infer as I
    kw = dict(RUNS[name])
    if kw.pop("align_draft", False):
        kw["align_draft"] = os.path.join(d, "drafts")
    out_dir = os.path.join(d, "out_" + name)
    saved = AL.EDITS_WORKSPACE_LIMIT, AL.windows_feasible
    if name == "edits_insertions":
        AL.EDITS_WORKSPACE_LIMIT = EDITS_LIMIT
    if name == "kernel_fallback":
        AL.windows_feasible = lambda *a: True
    text = io.StringIO()
    try:
        with contextlib.redirect_stdout(text):
            I.infer_folder(os.path.join(d, "wavs"), os.path.join(d, "config.yaml"), os.path.join(d, "best_model.pt"), out_dir,
                           confidence_threshold=CT, align="viterbi", **kw)
    finally:
        AL.EDITS_WORKSPACE_LIMIT, AL.windows_feasible = saved
    files = {}
    for f in sorted(os.listdir(out_dir)):
        with open(os.path.join(out_dir, f), "rb") as fh:
            files[f] = fh.read().decode("utf-8").replace(d, "<TMP>")
    return {"stdout": text.getvalue().replace(d, "<TMP>"), "files": files}


def run_all(d):
    build(d)
    return {name: run(d, name) for name in RUNS}
