"""The scenario of the `e2e` part of tests/golden/side_reports_e2e_parent.json (recorded by
tests/golden/make_side_reports_e2e_parent.py, held by tests/test_gpu_side_reports_identity.py): the tiny Whisper checkpoint of
label_viterbi_cases.build and one folder `side` of four files, one wave, run through infer_folder once per option set of RUNS and once
through infer_audio; every file a run writes and what it prints are the record.

  a.wav   7 s, a transcript of 32 tokens with the filler FILLER in the middle: aligned under filler_token; in the other two runs FILLER
          is a token the label set lacks, so the file falls back to the greedy alignment there
  b.wav   5 s, a transcript of 41 tokens without a filler (SP spelled): aligned in every run
  c.wav   3 s, a transcript with a token the label set lacks: never aligned
  d.wav   4 s, no transcript

The duration prior is written by hand as tests/test_gpu_align_duration_prior_scores_e2e.py writes its own: three soft histograms that
forbid nothing, and no row for p03 (its log_prior is `none`)."""
import contextlib
import io
import os

import numpy as np

import label_viterbi_cases as L
import synthetic as synth

FILLER = "<f>"
RUNS = {
    "optional": dict(optional_tokens="*", optional_scores=True),
    "filler": dict(filler_token=FILLER, filler_scores=True),
    "duration_prior": dict(duration_prior=True, duration_prior_scores=True),
}
AUDIO_RUN = "audio_filler"          # infer_audio of a.wav with RUNS["filler"]


def build(d):
    """label_viterbi_cases.build(d), then the folder `side` and the prior `prior.json` under the directory `d` (a str)."""
    from wfl_asr_amd import audio as A
    from wfl_asr_amd import durations as DU
    from wfl_asr_amd import postprocess as pp
    L.build(d)
    os.makedirs(os.path.join(d, "side"))
    a = L.transcript(30, seed=3)
    files = {"a": (810, 7, 0.9, a[:12] + [FILLER] + a[12:]), "b": (811, 5, 0.8, L.transcript(40, seed=5)),
             "c": (812, 3, 0.8, ["p00", "zz", "p01"]), "d": (813, 4, 0.7, None)}
    for name, (clip, sec, gain, tr) in files.items():
        A.write_wav(os.path.join(d, "side", name + ".wav"), synth.make_clip(clip, 16000 * sec, seed=L.SEED) * gain, 16000)
        if tr is not None:
            with open(os.path.join(d, "side", name + ".txt"), "w") as f:
                f.write(" ".join(tr))
    soft = [[-2.0, -1.0, -0.4, -1.5] + [-3.0] * 28, [-1.0, -0.5, -1.2, -2.0] + [-3.5] * 28, [-0.7, -0.7, -0.9] + [-4.0] * 29]
    DU.save(DU.DurationPrior(pp.FRAME_DURATION, 32, ["p00", "p01", "p02", "p03"], [np.asarray(r, np.float64) for r in soft] + [None],
                             np.asarray([-0.2, -0.4, -1.0, -np.inf], np.float64)), os.path.join(d, "prior.json"))


def _record(d, out_dir, call):
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        call()
    files = {}
    for f in sorted(os.listdir(out_dir)):
        with open(os.path.join(out_dir, f), "rb") as fh:
            files[f] = fh.read().decode("utf-8").replace(d, "<TMP>")
    return {"stdout": text.getvalue().replace(d, "<TMP>"), "files": files}


def run(d, name):
    """One run over the folder of build(d) -> {"stdout": what it printed, "files": {name: text of every file it wrote}}, the
    directory `d` spelled <TMP> in both."""
    from wfl_asr_amd import infer as I
    kw = dict(RUNS["filler" if name == AUDIO_RUN else name])
    if kw.get("duration_prior"):
        kw["duration_prior"] = os.path.join(d, "prior.json")
    kw.update(config_path=os.path.join(d, "config.yaml"), checkpoint_path=os.path.join(d, "best_model.pt"), confidence_threshold=L.CT,
              align="viterbi")
    out_dir = os.path.join(d, "out_" + name)
    if name == AUDIO_RUN:
        return _record(d, out_dir, lambda: I.infer_audio(os.path.join(d, "side", "a.wav"), output_lab_path=os.path.join(out_dir, "a.lab"),
                                                         **kw))
    return _record(d, out_dir, lambda: I.infer_folder(os.path.join(d, "side"), output_dir=out_dir, **kw))


def run_all(d):
    build(d)
    return {name: run(d, name) for name in list(RUNS) + [AUDIO_RUN]}
