"""The fixed rows and the fake Labeler of tests/golden/side_reports_parent.json (recorded by tests/golden/make_side_reports_parent.py at
the commit before wfl-asr_amd/reports.py, held by tests/test_side_reports_cpu.py).

ROWS: per kind four files of rows, as the plain field values of the kind's record.  a.wav and c.wav hold rows with equal sort keys,
in one file and across the two; b.wav has no flagged row (edits, insertions) and no row with a prior (durations); d.wav is empty.  Among
them: -inf ratios with "" names, log_prior None, the non-ASCII token "ñã", a FillerSpan without names.

GROUPS: the option sets that may be combined, and the kinds each one turns on.  canned(): what the fake Labeler._label_scored hands
back for the three files of the drivers' folder -- x.wav and z.wav aligned (the rows of a.wav and c.wav), y.wav not aligned."""
import contextlib
import io
import os

INF = float("inf")
RECORDS = {"edits": "TokenEdit", "insertions": "PlaceInsertion", "skipped": "SkippedToken", "optional": "OptionalTokenScore",
           "fillers": "FillerSpan", "filler_scores": "FillerScore", "durations": "TokenDuration"}
KINDS = list(RECORDS)

ROWS = {
    "edits": [
        ("a.wav", [[0, "p00", 0.0, 0.1234567, "p01", 1.5, "p02", -0.25, -3.0, 1],
                   [1, "ñã", 0.1234567, 0.5, "", -INF, "", -INF, -2.0, 0],
                   [2, "p02", 0.5, 0.75, "p03", 0.5, "p00", 1e-7, 1.5, 1],
                   [3, "p03", 0.75, 1.0, "p00", 123456.789, "", -INF, -1.0, 1]]),
        ("b.wav", [[0, "p01", 0.0, 0.2, "p00", -1.0, "p02", -2.0, -0.5, 0]]),
        ("c.wav", [[0, "p01", 0.02, 0.04, "p02", 1.5, "p03", 1.5, -4.0, 1],
                   [1, "SP", 0.04, 2.0000001, "p00", -0.000012345678, "p01", -7.0, 0.25, 1]]),
        ("d.wav", []),
    ],
    "insertions": [
        ("a.wav", [[0, "", "p00", 0.0, "p01", 2.0, "p02", 1.0, 1],
                   [1, "p00", "ñã", 0.1234567, "p03", 2.0, "p01", -0.5, 1],
                   [2, "ñã", "", 0.5, "", -INF, "", -INF, 0]]),
        ("b.wav", [[0, "", "p01", 0.0, "p00", -1.0, "p02", -2.5, 0], [1, "p01", "", 0.2, "p00", 0.0, "p03", -1e-9, 0]]),
        ("c.wav", [[0, "", "SP", 0.02, "p02", 3.25, "p03", 2.0, 1], [1, "SP", "", 2.0000001, "p00", 2.0, "p01", 1.999999, 1]]),
        ("d.wav", []),
    ],
    "skipped": [
        ("a.wav", [[1, "ñã", "p00", "p02", 0.1234567], [3, "p03", "p02", "", 1.0]]),
        ("b.wav", [[0, "p01", "", "", 0.0]]),
        ("c.wav", [[1, "SP", "p01", "", 2.0000001]]),
        ("d.wav", []),
    ],
    "optional": [
        ("a.wav", [[0, "p00", True, 0.75, 0.0, 0.1234567], [1, "ñã", False, 0.25, 0.1234567, 0.1234567],
                   [2, "p02", True, 0.4999995, 0.1234567, 0.5], [3, "p03", False, 0.5, 0.5, 0.5]]),
        ("b.wav", [[0, "p01", False, 0.9, 0.0, 0.0]]),
        ("c.wav", [[0, "p01", True, 0.75, 0.02, 0.04], [1, "SP", True, 1.0, 0.04, 2.0000001]]),
        ("d.wav", []),
    ],
    "fillers": [
        ("a.wav", [[1, 0.1234567, 0.5, 19, ["p01", "AP", "ñã"]], [3, 0.75, 1.0, 12, []]]),
        ("b.wav", [[0, 0.0, 0.2, 10, ["SP"]]]),
        ("c.wav", [[1, 0.04, 2.0000001, 98, ["p00", "p00"]]]),
        ("d.wav", []),
    ],
    "filler_scores": [
        ("a.wav", [[1, 0.1234567, 0.5, 19, 0.5, -0.01, 0.02, 0.03, 0.04], [3, 0.75, 1.0, 12, 0.5, 0.0, 0.0, -0.0000001, 1.25]]),
        ("b.wav", [[0, 0.0, 0.2, 10, 0.9999995, 0.001, 0.002, 0.003, 0.004]]),
        ("c.wav", [[1, 0.04, 2.0000001, 98, 0.5, 0.5, 0.25, -0.5, 0.125], [2, 2.0000001, 2.5, 25, 0.125, 0.0, 0.0, 0.0, 0.0]]),
        ("d.wav", []),
    ],
    "durations": [
        ("a.wav", [[0, "p00", 0.0, 0.1234567, 6, -1.5, 0.75, 0.01, 0.02, -0.03, 0.04, 5.25],
                   [1, "ñã", 0.1234567, 0.5, 19, None, 0.5, 0.0, 0.0, 0.0, 0.0, 19.0],
                   [2, "p02", 0.5, 0.75, 12, -1.5, 0.25, -0.001, 0.002, 0.003, 0.004, 12.00005],
                   [3, "p03", 0.75, 1.0, 13, -0.25, 1.0, 0.0, 0.0, 0.0, 0.0, 13.0]]),
        ("b.wav", [[0, "SP", 0.0, 0.2, 10, None, 0.9, 0.0, 0.1, 0.0, 0.1, 10.0]]),
        ("c.wav", [[0, "p01", 0.02, 0.04, 1, -1.5, 0.6, 0.0, 0.01, 0.0, 0.01, 1.0],
                   [1, "p02", 0.04, 2.0000001, 98, -30.123456789, 0.4, 0.5, 0.25, -0.5, 0.125, 48.0]]),
        ("d.wav", []),
    ],
}

GROUPS = {
    "plain": (dict(), []),
    "edits_insertions": (dict(align_edits=True, align_insertions=True), ["edits", "insertions"]),
    "optional": (dict(optional_tokens="*", optional_scores=True), ["skipped", "optional"]),
    "filler": (dict(filler_token="<f>", filler_scores=True), ["fillers", "filler_scores"]),
    "duration_prior": (dict(duration_prior="prior.json", duration_prior_scores=True), ["durations"]),
}
WORLDS = {"world1": {"RANK": "0", "WORLD_SIZE": "1"}, "rank1of2": {"RANK": "1", "WORLD_SIZE": "2"}}
FOLDER = {"x.wav": 300, "y.wav": 200, "z.wav": 100}            # the drivers' folder: name -> bytes
_CANNED_FROM = {"x.wav": "a.wav", "z.wav": "c.wav"}             # y.wav: not aligned


def records(kind, rows):
    """The rows of ROWS (or of the JSON) as the kind's records."""
    from wfl_asr_amd import align as AL
    cls = getattr(AL, RECORDS[kind])
    return [cls(*(tuple(v) if isinstance(v, list) else v for v in r)) for r in rows]


def per_file(kind):
    return [(name, records(kind, rows)) for name, rows in ROWS[kind]]


def canned(audio_paths, opts, kinds):
    """-> (segments, scores, {kind: {file index: rows}}) of the fake _label_scored for the files `audio_paths`."""
    from wfl_asr_amd import align as AL
    final, scores, rows = [], [], {kind: {} for kind in kinds}
    for fi, p in enumerate(audio_paths):
        name = os.path.basename(p)
        src = _CANNED_FROM.get(name)
        final.append([(0.0, 0.25 + 0.01 * len(name), "p00"), (0.25 + 0.01 * len(name), 0.5, "SP")] if src else [(0.0, 0.5, "AP")])
        scores.append(AL.FileScore(-1.25, -0.5, -0.45, 0.25, [AL.TokenScore("p00", 0.0, 0.26, 0.25, 0.01, -0.002)])
                      if src and opts.scored else None)
        for kind in kinds:
            if src:
                rows[kind][fi] = records(kind, dict(ROWS[kind])[src])
    return final, scores, rows


def plain(x):
    """A label_files result as JSON holds it: records and tuples as lists."""
    if isinstance(x, (list, tuple)):
        return [plain(v) for v in x]
    return x


def _written(d):
    """Every file under the drivers' two output directories: {path relative to d: text}."""
    files = {}
    for sub in ("out", "one"):
        for f in sorted(os.listdir(os.path.join(d, sub))):
            with open(os.path.join(d, sub, f), "rb") as fh:
                files[sub + "/" + f] = fh.read().decode("utf-8").replace(d, "<TMP>")
    return files


def drive(I, d, group):
    """infer_folder over the folder FOLDER, then infer_audio of x.wav and of y.wav, with I._labeler already patched to hand out
    the fake Labeler; under the directory `d` (a str, empty) -> {"stdout", "files"}, the directory spelled <TMP>.  The environment (RANK,
    WORLD_SIZE) is the caller's."""
    given = dict(GROUPS[group][0], align="viterbi")
    os.makedirs(os.path.join(d, "wavs"))
    for name, size in FOLDER.items():
        with open(os.path.join(d, "wavs", name), "wb") as f:
            f.write(b"\0" * size)
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        I.infer_folder(os.path.join(d, "wavs"), os.path.join(d, "no_config.yaml"), "no_model.pt", os.path.join(d, "out"), **given)
        for stem in ("x", "y"):
            I.infer_audio(os.path.join(d, "wavs", stem + ".wav"), os.path.join(d, "no_config.yaml"), "no_model.pt",
                          os.path.join(d, "one", stem + ".lab"), **given)
    return {"stdout": text.getvalue().replace(d, "<TMP>"), "files": _written(d)}
