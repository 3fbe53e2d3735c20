"""CPU (-m "not gpu"), no build: options.resolve, the one place where the post-processing options of a request are resolved
(argument, else config `postprocess.<key>`, else default) and the rules between them are applied, in one fixed order.  The tables
hold the cases that used to bind the Labeler's option methods onto a stub (same config, same arguments, same expectations)."""
import dataclasses
import math

import pytest

from wfl_asr_amd import options as O
from wfl_asr_amd.options import PostOptions, resolve

BG = {"decode": "viterbi", "phoneme_bigram": "bg.json"}
NAN = float("nan")

# (config postprocess section, arguments, the fields that are checked)
ACCEPTED = [
    # align
    ({}, {}, dict(align="greedy")),
    ({"align": "viterbi"}, {}, dict(align="viterbi")),
    ({"align": "viterbi"}, dict(align="greedy"), dict(align="greedy")),
    # align_scores
    ({}, {}, dict(align_scores=False)),
    ({"align": "viterbi"}, {}, dict(align_scores=False)),
    ({"align": "viterbi", "align_scores": True}, {}, dict(align_scores=True)),
    ({"align": "viterbi", "align_scores": True}, dict(align_scores=False), dict(align_scores=False)),
    ({}, dict(align_scores=True, align="viterbi"), dict(align_scores=True)),
    # decode, switch_penalty
    ({}, {}, dict(decode="argmax", switch_penalty=0.0)),
    ({"decode": "viterbi", "switch_penalty": 2}, {}, dict(decode="viterbi", switch_penalty=2.0)),
    ({"decode": "viterbi", "switch_penalty": 2}, dict(decode="argmax", switch_penalty=0.5), dict(decode="argmax", switch_penalty=0.5)),
    ({}, dict(decode="viterbi", switch_penalty=4), dict(decode="viterbi", switch_penalty=4.0)),
    # decode_scores
    ({}, {}, dict(decode_scores=False)),
    ({"decode": "viterbi"}, {}, dict(decode_scores=False)),
    ({"decode": "viterbi", "decode_scores": True}, {}, dict(decode_scores=True)),
    ({"decode": "viterbi", "decode_scores": True}, dict(decode_scores=False), dict(decode_scores=False)),
    ({}, dict(decode_scores=True, decode="viterbi"), dict(decode_scores=True)),
    # phoneme_bigram, bigram_weight
    ({}, {}, dict(phoneme_bigram=None, bigram_weight=1.0)),
    ({**BG, "bigram_weight": 0.5}, {}, dict(phoneme_bigram="bg.json", bigram_weight=0.5)),
    ({"decode": "viterbi"}, dict(phoneme_bigram="x.json"), dict(phoneme_bigram="x.json", bigram_weight=1.0)),
    # bigram_scores: accepted with a bigram, by the config key as by the argument
    ({}, {}, dict(bigram_scores=False)),
    (BG, {}, dict(bigram_scores=False)),
    ({**BG, "bigram_scores": True}, {}, dict(bigram_scores=True)),
    (BG, dict(bigram_scores=True), dict(bigram_scores=True)),
    ({"decode": "viterbi"}, dict(bigram_scores=True, phoneme_bigram="bg.json"), dict(bigram_scores=True)),
    ({}, dict(bigram_scores=True, phoneme_bigram="bg.json", decode="viterbi"), dict(bigram_scores=True)),
    ({**BG, "bigram_scores": True}, dict(bigram_scores=False), dict(bigram_scores=False)),
    ({**BG, "bigram_scores": True}, {}, dict(phoneme_bigram="bg.json", bigram_weight=1.0)),
    # the argument wins, also over a config value that would be refused on its own
    ({"align": "best", "decode": "beam", "switch_penalty": -1}, dict(align="viterbi", decode="viterbi", switch_penalty=2),
     dict(align="viterbi", decode="viterbi", switch_penalty=2.0)),
    # an empty path is no bigram, and as an argument it takes the config's away
    ({"phoneme_bigram": ""}, {}, dict(phoneme_bigram=None)),
    (BG, dict(phoneme_bigram=""), dict(phoneme_bigram=None)),
]

# (config postprocess section, arguments, match): inputs that break one rule
REFUSED = [
    ({}, dict(align="nearest"), "align"),
    ({"align": "best"}, {}, "align"),
    ({}, dict(align_scores=True), "align_scores"),
    ({"align": "viterbi"}, dict(align_scores=True, align="greedy"), "align_scores"),
    ({"align_scores": True}, {}, "align_scores"),
    ({}, dict(decode="median"), "decode"),
    ({"decode": "best"}, {}, "decode"),
    ({"switch_penalty": -0.1}, {}, "switch_penalty"),
    ({}, dict(decode="viterbi", switch_penalty=NAN), "switch_penalty"),
    ({}, dict(switch_penalty="much"), "switch_penalty"),
    ({}, dict(switch_penalty=True), "switch_penalty must be a number >= 0"),
    ({}, dict(decode_scores=True), "the argmax decode has no lattice to score"),
    ({"decode": "viterbi"}, dict(decode_scores=True, decode="argmax"), "the argmax decode has no lattice to score"),
    ({"decode_scores": True}, {}, "the argmax decode has no lattice to score"),
    ({"phoneme_bigram": "bg.json"}, {}, "need decode='viterbi'"),
    ({"decode": "viterbi"}, dict(phoneme_bigram="bg.json", decode="argmax"), "need decode='viterbi'"),
    ({}, dict(bigram_weight=1.0), "need decode='viterbi'"),
    ({**BG, "bigram_weight": -0.5}, {}, "bigram_weight must be a number >= 0"),
    (BG, dict(bigram_weight=True), "bigram_weight must be a number >= 0"),
    ({**BG, "decode_scores": True}, {}, "decode_scores cannot be combined with a phoneme bigram.*bigram_scores"),
    ({"decode": "viterbi"}, dict(phoneme_bigram="bg.json", decode_scores=True),
     "decode_scores cannot be combined with a phoneme bigram.*bigram_scores"),
    ({**BG, "bigram_scores": True}, dict(decode_scores=True), "decode_scores cannot be combined with a phoneme bigram.*bigram_scores"),
    ({"decode": "viterbi", "bigram_scores": True}, {}, "bigram_scores needs a phoneme_bigram"),
    ({"decode": "viterbi"}, dict(bigram_scores=True), "bigram_scores needs a phoneme_bigram"),
    ({}, dict(bigram_scores=True), "bigram_scores needs decode='viterbi'"),
    ({"bigram_scores": True}, {}, "bigram_scores needs decode='viterbi'"),
]

# (config postprocess section, arguments, rule reported, rule also broken, match): the earlier rule of the fixed order is the one
# that is reported.  Rules 8 and 9 need what the other forbids (a bigram under decode viterbi), so they are only ever the later one.
ORDER = [
    ({}, dict(align="dtw", decode="beam"), 1, 3, "align must be one of"),
    ({}, dict(align_scores=True, decode="beam"), 2, 3, "align_scores needs align='viterbi'"),
    ({}, dict(decode="beam", switch_penalty=-1), 3, 4, "decode must be one of"),
    ({}, dict(switch_penalty=-1, decode_scores=True), 4, 5, "switch_penalty must be a number >= 0"),
    ({}, dict(decode_scores=True, bigram_weight=-1), 5, 6, "decode_scores needs decode='viterbi'"),
    ({}, dict(bigram_weight=-1, phoneme_bigram="bg.json"), 6, 7, "bigram_weight must be a number >= 0"),
    # (the two cases that the bigram_scores method, called alone, used to answer with its own rule)
    (BG, dict(bigram_scores=True, decode="argmax"), 7, 9, "need decode='viterbi'"),
    ({"bigram_scores": True}, dict(phoneme_bigram="bg.json"), 7, 9, "need decode='viterbi'"),
    (BG, dict(bigram_weight=-1, decode_scores=True), 6, 8, "bigram_weight must be a number >= 0"),
    (BG, dict(switch_penalty=-1, decode_scores=True), 4, 8, "switch_penalty must be a number >= 0"),
    ({}, dict(decode_scores=True, bigram_scores=True), 5, 9, "decode_scores needs decode='viterbi'"),
    ({"decode": "viterbi"}, dict(align="dtw", bigram_scores=True), 1, 9, "align must be one of"),
]


@pytest.mark.parametrize("post, given, want", ACCEPTED)
def test_accepted(post, given, want):
    opts = resolve(post, **given)
    assert isinstance(opts, PostOptions)
    for name, value in want.items():
        got = getattr(opts, name)
        assert got == value and type(got) is type(value), (name, got)


@pytest.mark.parametrize("post, given, match", REFUSED)
def test_refused(post, given, match):
    with pytest.raises(ValueError, match=match):
        resolve(post, **given)


@pytest.mark.parametrize("post, given, first, later, match", ORDER)
def test_the_earlier_rule_is_reported(post, given, first, later, match):
    assert first < later
    with pytest.raises(ValueError, match=match):
        resolve(post, **given)


def test_the_record():
    assert PostOptions._fields == ("align", "align_scores", "decode", "switch_penalty", "decode_scores", "phoneme_bigram",
                                   "bigram_weight", "bigram_scores")
    d = resolve(None)
    assert d == resolve({}) == PostOptions("greedy", False, "argmax", 0.0, False, None, 1.0, False)
    assert d.free_scores is False and d.scored is False
    with pytest.raises((AttributeError, dataclasses.FrozenInstanceError)):
        d.align = "viterbi"
    a = resolve({}, align="viterbi", align_scores=True)
    assert a.scored and not a.free_scores
    f = resolve({}, decode="viterbi", decode_scores=True)
    assert f.scored and f.free_scores
    b = resolve(BG, bigram_scores=True, switch_penalty="2")
    assert b.scored and b.free_scores and not b.decode_scores and b.switch_penalty == 2.0
    assert math.isinf(resolve({}, switch_penalty=float("inf")).switch_penalty)
    assert O.ALIGN_MODES == ("greedy", "viterbi") and O.DECODE_MODES == ("argmax", "viterbi")
    with pytest.raises(ValueError) as e:
        resolve(BG, decode_scores=True)
    assert str(e.value) == O.BIGRAM_SCORES_ERROR
    with pytest.raises(TypeError):
        resolve({}, "viterbi")                          # the options are keyword-only
