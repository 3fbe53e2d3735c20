"""-m gpu: `postprocess.transcript_variants` end to end on the synthetic tiny Whisper checkpoint of test_gpu_align_min_duration_e2e.py
(random weights, rebuilt here): a file whose transcript holds groups gives the segments of the float64 graph DP over the forward's own
logits and its VariantChoice rows; in a folder where some transcripts carry groups and some do not, the .lab of a file without groups is
byte for byte the .lab of the run without the option, each group's chosen variant stands in the .lab, the .variants.tsv rows agree with
it, the gain is >= -1e-3 T, transcript_variants.tsv is sorted, a file whose groups leave it no path falls back with the message, and
with the key absent no new call is made and no new file written."""
import os
import shutil

import numpy as np
import pytest
import torch

import viterbi_graph_ref as G
from test_gpu_align_e2e import LABELS
from test_gpu_align_min_duration_e2e import CT, FD, _bytes, _transcript, whisper  # noqa: F401  (the module's fixture, built once here)
from wfl_asr_amd import align as AL
from wfl_asr_amd import infer as I
from wfl_asr_amd import reports as RP

pytestmark = pytest.mark.gpu


def _with_groups(base, groups):
    """The words of a transcript: `base` with the text of groups[i] put in at word i."""
    out = []
    for i, t in enumerate(base):
        if i in groups:
            out += groups[i].split()
        out.append(t)
    return out


WORDS_A = _with_groups(_transcript(60), {0: "( p00 | p01 )", 20: "( p02 | )", 45: "(p01 p03|p02|p00 p00 p01)"})
WORDS_B = _with_groups(_transcript(50, seed=8), {10: "( p03 | p00 p01 )", 49: "( p02 p02 | )"})


def _write(path, words):
    with open(path.replace(".wav", ".txt"), "w") as f:
        f.write(" ".join(words))


def _host_reference(lab, path, graph):
    """The clip through model.label(want_logits=True) and the float64 graph DP, assembled by the host helpers -> (segments, taken, the
    DP's score minus the score of the transcript as written, frames)."""
    chunks = lab._load_chunks(path)
    assert len(chunks) == 1
    x = np.zeros((lab.batch_size, lab.chunk_samples), np.float32)
    x[0, :len(chunks[0])] = chunks[0]
    lens = np.zeros(lab.batch_size, np.int32)
    lens[0] = len(chunks[0])
    res = lab.model.label(torch.from_numpy(x).cuda(), None, threshold=CT, lens=lens, average_languages=True, want_logits=True)
    tv = lab._valid_frames(len(chunks[0]), res.ids.shape[1])
    z = res.logits[0, :tv].cpu().numpy()
    offs = res.offsets[0, :tv].cpu().numpy()
    remap, names = lab._names_for(None)
    alts, why = AL.token_alternatives(graph.slots, lab._table, remap, names, LABELS)
    assert why is None
    gaps = AL.gap_classes(LABELS, graph.slots)
    states, score = G.viterbi(z, alts, graph.preds, graph.final, gaps)
    assert states is not None
    ids, tok, taken = G.outputs(states, z, alts, LABELS.index("O"))
    _, written = G.V.viterbi(z, [alts[k] for k in graph.first], gaps)
    segs = AL.path_segments(ids, tok, [tv], [offs], [0.0], lab._table, alts, graph.slots, FD, skipped=1 - taken)
    return segs, taken, score - written, tv


def test_a_file_with_groups_gives_the_host_graph_dp(whisper, monkeypatch, capsys):  # noqa: F811
    d, lab = whisper
    path = str(d / "wavs" / "a.wav")
    graph = AL.compile_graph(AL.parse_variants(WORDS_A))
    ref, taken, ref_gain, T = _host_reference(lab, path, graph)
    calls = []
    real = AL.viterbi_align_graph
    monkeypatch.setattr(AL, "viterbi_align_graph", lambda *a, **kw: calls.append(a) or real(*a, **kw))
    _write(path, WORDS_A)
    try:
        capsys.readouterr()
        final, variants = lab.label_files([path], confidence_threshold=CT, align="viterbi", transcript_variants=True)
        out = capsys.readouterr().out
        assert len(calls) == 1
        assert final[0] == ref and [s[2] for s in final[0]] == [n for n, f in zip(graph.slots, taken) if f]
        rows = variants[0]
        assert rows == AL.variant_choices(graph, taken, ref, rows[0].gain) and len(rows) == 3
        assert abs(rows[0].gain - ref_gain) <= 2e-3 * T and rows[0].gain >= -1e-3 * T
        assert f"3 groups, {sum(r.choice != 0 for r in rows)} not as written, gain {rows[0].gain:.3f} nats" in out
        # without the key: `(` is a token like any other, as it was -- no graph call, the greedy alignment with its line
        plain = lab.label_files([path], confidence_threshold=CT, align="viterbi")
        out = capsys.readouterr().out
        assert len(calls) == 1 and isinstance(plain, list) and "token '(' matches no phoneme" in out
        # a malformed transcript is refused, naming the file and the place; so are the options whose lattices are chains
        _write(path, WORDS_A + "( p00 | ( p01 | p02 ) )".split())
        with pytest.raises(ValueError, match=r"a\.txt: word \d+: a group inside the group opened at word \d+"):
            lab.label_files([path], confidence_threshold=CT, align="viterbi", transcript_variants=True)
        with pytest.raises(ValueError, match="transcript_variants cannot be combined with align_scores:"):
            lab.label_files([path], confidence_threshold=CT, align="viterbi", transcript_variants=True, align_scores=True)
    finally:
        os.remove(path.replace(".wav", ".txt"))


def _lab_rows(path):
    with open(path, encoding="utf-8") as f:
        return [(int(a), int(b), n) for a, b, n in (ln.split() for ln in f if ln.strip())]


def test_a_folder_with_and_without_groups(whisper, tmp_path, monkeypatch, capsys):  # noqa: F811
    d, lab = whisper
    folder = tmp_path / "in"
    os.makedirs(folder)
    for name, src in [("a", "a"), ("b", "a"), ("c", "plain"), ("plain", "plain")]:
        shutil.copyfile(str(d / "wavs" / f"{src}.wav"), str(folder / f"{name}.wav"))
    plain_tr = _transcript(40, seed=9)
    no_path = _with_groups(_transcript(260, seed=10), {5: "( p00 | p01 p02 )"})      # 262 slots at least, 200 frames
    for name, words in [("a", WORDS_A), ("b", WORDS_B), ("c", no_path), ("plain", plain_tr)]:
        _write(str(folder / f"{name}.wav"), words)
    calls = []
    real = AL.viterbi_align_graph
    monkeypatch.setattr(AL, "viterbi_align_graph", lambda *a, **kw: calls.append(a) or real(*a, **kw))
    args = [str(folder), "-ckpt", str(d / "best_model.pt"), "-c", str(d / "config.yaml"), "--align", "viterbi"]
    capsys.readouterr()
    with pytest.raises(SystemExit) as e:
        I.main(args + ["-o", str(tmp_path / "without")])
    assert e.value.code == 0 and calls == []
    assert sorted(os.listdir(tmp_path / "without")) == ["a.lab", "b.lab", "c.lab", "plain.lab"]
    capsys.readouterr()
    with pytest.raises(SystemExit) as e:
        I.main(args + ["-o", str(tmp_path / "with"), "--transcript-variants"])
    out = capsys.readouterr().out
    assert e.value.code == 0 and len(calls) == 1
    assert sorted(os.listdir(tmp_path / "with")) == ["a.lab", "a.variants.tsv", "b.lab", "b.variants.tsv", "c.lab", "plain.lab",
                                                     "transcript_variants.tsv"]
    # a file without groups: byte for byte the .lab of the run without the option
    assert open(tmp_path / "with" / "plain.lab", "rb").read() == open(tmp_path / "without" / "plain.lab", "rb").read()
    assert [n for _, _, n in _lab_rows(tmp_path / "with" / "plain.lab")] == plain_tr
    # a file whose groups leave it no path: the message, and the greedy alignment of the transcript as written
    assert "c.wav: viterbi alignment not possible (no way through the 1 groups' variants fits 200 frames); using the greedy alignment" in out
    gains = {}
    for name, words, T in [("a", WORDS_A, 350), ("b", WORDS_B, 350)]:
        graph = AL.compile_graph(AL.parse_variants(words))
        lab_rows = _lab_rows(tmp_path / "with" / f"{name}.lab")
        with open(tmp_path / "with" / f"{name}.variants.tsv", encoding="utf-8") as f:
            lines = f.read().split("\n")
        assert lines[0] == RP.KINDS["variants"].header and lines[-1] == "" and len(lines) == len(graph.groups) + 2
        rows = [ln.split("\t") for ln in lines[1:-1]]
        # each group's chosen variant stands in the .lab: the .lab spells the expansion the rows choose
        chosen = {int(r[0]): int(r[3]) for r in rows}
        spelled, gi = [], 0
        for el in graph.elements:
            if isinstance(el, str):
                spelled.append(el)
            else:
                spelled += list(el[chosen[gi]])
                gi += 1
        assert [n for _, _, n in lab_rows] == spelled
        # the rows agree with the .lab: spelling, as written, and the chosen variant's time
        k = 0
        gi = 0
        for el in graph.elements:
            if isinstance(el, str):
                k += 1
                continue
            r = rows[gi]
            var = el[chosen[gi]]
            assert r[4] == " ".join(var) and r[5] == " ".join(el[0])
            start, end = round(float(r[1]) * 1e7), round(float(r[2]) * 1e7)
            if var:
                assert abs(start - lab_rows[k][0]) <= 1 and abs(end - lab_rows[k + len(var) - 1][1]) <= 1
            else:
                assert start == end and abs(start - (lab_rows[k][0] if k < len(lab_rows) else lab_rows[-1][1])) <= 1
            k += len(var)
            gi += 1
        assert len({r[6] for r in rows}) == 1
        gains[name] = float(rows[0][6])
        assert gains[name] >= -1e-3 * T
        assert f"{name}.wav: {len(rows)} groups, {sum(c != 0 for c in chosen.values())} not as written, gain" in out
    # the folder file: the groups whose choice is not the first variant, the file with the largest gain first
    with open(tmp_path / "with" / "transcript_variants.tsv", encoding="utf-8") as f:
        lines = f.read().split("\n")
    assert lines[0] == "file\t" + RP.KINDS["variants"].header
    body = [ln.split("\t") for ln in lines[1:-1]]
    assert all(r[4] != "0" for r in body) and {r[0] for r in body} <= {"a.wav", "b.wav"}
    order = [float(r[7]) for r in body]
    assert order == sorted(order, reverse=True) and all(float(r[7]) == pytest.approx(gains[r[0][0]], abs=1e-4) for r in body)
