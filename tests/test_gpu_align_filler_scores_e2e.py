"""-m gpu: `postprocess.filler_scores` end to end, on the synthetic tiny Whisper checkpoint and the clips of
test_gpu_align_filler_e2e.py: with the option the .lab, .fillers.tsv and filler_spans.tsv are byte for byte what they are without it;
{stem}.scores.tsv, {stem}.filler_scores.tsv, alignment_scores.tsv and filler_scores.tsv exist with their columns, one filler row per
filler; a file without a filler in the same folder is scored on the lattice it was searched on, and its scores.tsv is what
align_scores writes for it without a filler_token; --filler-scores without --filler-token is refused with the option's own message."""
import os
import shutil

import pytest

from test_gpu_align_e2e import _write_tr
from test_gpu_align_filler_e2e import F, _with_filler
from test_gpu_align_min_duration_e2e import CT, _transcript, whisper  # noqa: F401  (the module's fixture, built once here)
from wfl_asr_amd import align as AL
from wfl_asr_amd import infer as I
from wfl_asr_amd import options as O
from wfl_asr_amd import reports as RP

pytestmark = pytest.mark.gpu


def _read(p):
    with open(p, "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def folders(whisper, tmp_path_factory):  # noqa: F811
    """One folder, a.wav with a filler in its transcript and b.wav (the same audio) without, labelled three times through the CLI:
    with --filler-token, with --filler-token --filler-scores, and with --align-scores alone (b.wav only)."""
    d, lab = whisper
    root = tmp_path_factory.mktemp("filler_scores")
    folder = root / "in"
    os.makedirs(folder)
    for name in ("a.wav", "b.wav"):
        shutil.copyfile(str(d / "wavs" / "a.wav"), str(folder / name))
    _write_tr(str(folder / "a.wav"), _with_filler(_transcript(90)))
    _write_tr(str(folder / "b.wav"), _transcript(90))
    args = [str(folder), "-ckpt", str(d / "best_model.pt"), "-c", str(d / "config.yaml"), "--align", "viterbi", "-ct", str(CT)]
    outs = {}
    for key, extra in (("plain", ["--filler-token", F]), ("scored", ["--filler-token", F, "--filler-scores"])):
        with pytest.raises(SystemExit) as e:
            I.main(args + ["-o", str(root / key)] + extra)
        assert e.value.code == 0
        outs[key] = root / key
    only_b = root / "in_b"
    os.makedirs(only_b)
    shutil.copyfile(str(folder / "b.wav"), str(only_b / "b.wav"))
    _write_tr(str(only_b / "b.wav"), _transcript(90))
    with pytest.raises(SystemExit) as e:
        I.main([str(only_b)] + args[1:] + ["-o", str(root / "align_scores"), "--align-scores"])
    assert e.value.code == 0
    outs["align_scores"] = root / "align_scores"
    return outs, args


def test_the_lab_and_the_span_files_are_byte_identical(folders):
    outs, _ = folders
    plain = sorted(os.listdir(outs["plain"]))
    assert plain == ["a.fillers.tsv", "a.lab", "b.lab", "filler_spans.tsv"]
    for name in plain:
        assert _read(outs["plain"] / name) == _read(outs["scored"] / name), name


def test_the_new_files_and_their_columns(folders):
    outs, _ = folders
    assert sorted(os.listdir(outs["scored"])) == ["a.filler_scores.tsv", "a.fillers.tsv", "a.lab", "a.scores.tsv", "alignment_scores.tsv",
                                                  "b.filler_scores.tsv", "b.lab", "b.scores.tsv", "filler_scores.tsv", "filler_spans.tsv"]
    rows = _read(outs["scored"] / "a.filler_scores.tsv").decode().splitlines()
    assert rows[0] == RP.REPORTS["filler_scores"].header and rows[0].split("\t") == ["index", "start_s", "end_s", "frames", "posterior", "start_shift_s",
                                                                          "start_sd_s", "end_shift_s", "end_sd_s"]
    assert len(rows) == 2                                     # one filler in the transcript
    cells = rows[1].split("\t")
    span = _read(outs["scored"] / "a.fillers.tsv").decode().splitlines()[1].split("\t")
    assert cells[:4] == span[:4] and cells[0] == "30" and int(cells[3]) >= 1
    assert 0.0 <= float(cells[4]) <= 1.0 and float(cells[6]) >= 0.0 and float(cells[8]) >= 0.0
    assert _read(outs["scored"] / "b.filler_scores.tsv").decode().splitlines() == [RP.REPORTS["filler_scores"].header]      # no filler, no row
    folder_rows = _read(outs["scored"] / "filler_scores.tsv").decode().splitlines()
    assert folder_rows == ["file\t" + RP.REPORTS["filler_scores"].header, "a.wav\t" + rows[1]]
    # {stem}.scores.tsv: align_scores' format, one row per transcript token, the filler's row under its NAME with its span
    tr = _with_filler(_transcript(90))
    sc = [r.split("\t") for r in _read(outs["scored"] / "a.scores.tsv").decode().splitlines() if not r.startswith("#")]
    assert [r[2] for r in sc] == tr and all(len(r) == 6 for r in sc)
    assert sc[30][2] == F and abs(int(sc[30][0]) - float(span[1]) * 1e7) <= 1 and abs(int(sc[30][1]) - float(span[2]) * 1e7) <= 1
    assert all(0.0 <= float(r[3]) <= 1.0 for r in sc)
    review = _read(outs["scored"] / "alignment_scores.tsv").decode()
    assert "a.wav" in review and "b.wav" in review


def test_a_file_without_a_filler_is_scored_as_align_scores_scores_it(folders):
    outs, _ = folders
    assert _read(outs["scored"] / "b.scores.tsv") == _read(outs["align_scores"] / "b.scores.tsv")
    assert _read(outs["scored"] / "b.lab") == _read(outs["align_scores"] / "b.lab")


def test_filler_scores_without_a_filler_token_is_refused(folders, monkeypatch, capsys):
    _, args = folders
    monkeypatch.setattr(I, "_labeler", lambda *a, **kw: pytest.fail("a model was loaded"))
    with pytest.raises(SystemExit) as e:
        I.main(args + ["--filler-scores"])
    assert e.value.code != 0
    assert "filler_scores needs a filler_token" in capsys.readouterr().err and "align_scores is the option to ask for" in O.FILLER_SCORES_ERROR
    with pytest.raises(ValueError, match="filler_scores needs a filler_token"):
        I.infer_folder(folder_path=args[0], config_path=args[4], checkpoint_path=args[2], align="viterbi", filler_scores=True)
