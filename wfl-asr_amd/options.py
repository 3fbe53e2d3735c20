"""The post-processing options of a labelling request, resolved once: argument, else the config's `postprocess.<key>`, else the
default, then the rules between the options, in one fixed order with one message each.  Pure Python: the Labeler, infer_audio /
infer_folder (before any model is loaded) and the CLI all call `resolve` and carry the `PostOptions` record it returns.

  option          default   rule (checked in this order; the first broken one is reported)
  align           greedy    1. one of ALIGN_MODES
  align_scores    off       2. needs align viterbi
  decode          argmax    3. one of DECODE_MODES
  switch_penalty  0         4. a number >= 0 (no bool, no NaN, no string that is not a number)
  decode_scores   off       5. needs decode viterbi
  bigram_weight   1         6. when given, a number >= 0 (no bool)
  phoneme_bigram  none      7. a phoneme_bigram or a given bigram_weight needs decode viterbi
                            8. decode_scores with a phoneme_bigram is refused (BIGRAM_SCORES_ERROR): a posterior must score the
                               grammar its search ran on, and decode_scores' pass knows the flat switch penalty only
  bigram_scores   off       9. needs decode viterbi, and then a phoneme_bigram
  align_draft     none     10. needs align viterbi (the draft's windows hold that search)
  draft_tolerance 0.1      11. when given, a number >= 0 (seconds; no bool), and then needs an align_draft
  align_edits     off      12. needs align viterbi (the edits are scored on the lattice of that search)
  align_insertions off     13. needs align viterbi (the insertions are scored on the lattice of that search)
  min_duration    none     14. SECONDS or {NAME: SECONDS, default: SECONDS}: every value a number between 0 and
                               MAX_MIN_FRAMES * FRAME_DURATION (no bool)
                           15. needs align viterbi (the durations constrain that search)
                           16. align_scores, align_edits and align_insertions beside a min_duration are refused
                               (MIN_DURATION_SCORES_ERROR): their passes score the lattice without minimum durations, and a score must
                               speak of the lattice its search ran on
  duration_scores off      17. needs align viterbi
                           18. needs a min_duration (it scores the minimum-duration lattice; without durations align_scores is the
                               option to ask for)
  optional_tokens none    19. [NAME, ...] or "*": a list of token names (strings), or the string "*" for every token
                           20. needs align viterbi (the skip arcs are arcs of that search)
  skip_penalty    0        21. when given, a number >= 0 (nats per skipped token; no bool, no NaN)
                           22. when given, needs optional_tokens (it is the price of skipping one)
                           23. min_duration, align_scores, align_edits, align_insertions and duration_scores beside optional_tokens
                               are refused (OPTIONAL_TOKENS_ERROR): their lattices have no skip arcs, and a score must speak of the
                               lattice its search ran on
                           (24. with the model known, Labeler.label_files: a name that is no output name of the label set is refused
                               by name, `unknown_optional_tokens`)
  optional_scores off      25. needs align viterbi
                           26. needs optional_tokens (it scores the skip lattice of that search: per optional token the posterior
                               that it is present; without optional tokens align_scores is the option to ask for)
  filler_token    none    27. NAME: a non-empty string without whitespace; a transcript token equal to it matches anything
                           28. needs align viterbi (the filler is a token of that search)
  filler_penalty  1.0      29. when given, a finite number >= 0 (nats per frame of a filler's run; no bool, no NaN).  The default of 1.0
                               is a value to start from, not a measured optimum
                           30. when given, needs a filler_token (it is the price per frame of that token)
                           31. align_draft, min_duration, optional_tokens, align_scores, align_edits, align_insertions,
                               duration_scores and optional_scores beside a filler_token are refused (FILLER_TOKEN_ERROR): their
                               lattices have no filler emission, and a score must speak of the lattice its search ran on
                           (32. with the model known, Labeler.label_files: a filler_token that is an output name of the label set is
                               refused by name, `filler_token_collision`)
  filler_scores   off      33. a bool (true / false; no number, no string)
                           34. needs a filler_token (it scores the filler lattice of that search: per filler the posterior of its
                               span and the spread of both its ends; without a filler_token align_scores is the option to ask for)
  duration_prior  none    35. PATH of a phoneme_durations.json (python -m wfl_asr_amd.durations); needs align viterbi (the prior is a
                               term of that search's path score)
  duration_prior_weight 1.0  36. when given, a finite number >= 0 (no bool, no NaN): the table is weight * log P.  The default of 1.0 is
                               a value to start from, not a measured optimum
                           37. when given, needs a duration_prior (it scales that prior)
                           38. align_draft, min_duration, optional_tokens, filler_token, align_scores, align_edits,
                               align_insertions, duration_scores, optional_scores and filler_scores beside a duration_prior are
                               refused (DURATION_PRIOR_ERROR): their lattices carry no duration term, and a search or a score must
                               speak of one lattice
                           (39. with the model known, Labeler.label_files: a file counted on another frame duration, or one that
                               holds a phoneme that is no output name of the label set, is refused by name, durations.check)
  duration_prior_scores off 40. a bool (true / false; no number, no string)
                           41. needs a duration_prior (it scores the explicit-duration lattice of that search: per token the
                               posterior of its run, the spread of both its ends and its expected length; without a prior
                               align_scores is the option to ask for)
  decode_duration_prior none 42. PATH of a phoneme_durations.json; a decode_duration_prior or a given decode_duration_prior_weight needs
                               decode viterbi (the prior is a term of the free decode's path score: the explicit-duration search
                               wfl_decode_duration, under the phoneme_bigram's table where one is given, else the flat switch
                               penalty).  `duration_prior` stays the transcript alignment's prior
  decode_duration_prior_weight 1.0  43. when given, a finite number >= 0 (no bool, no NaN): the table is weight * log P.  The default of
                               1.0 is a value to start from, not a measured optimum
                           44. when given, needs a decode_duration_prior (it scales that prior)
                           45. decode_scores and bigram_scores beside a decode_duration_prior are refused
                               (DECODE_DURATION_PRIOR_ERROR): their sweeps carry no duration term, and a posterior must score the
                               grammar its search ran on
                           (46. with the model known, Labeler.label_files: durations.check, as rule 39)
  decode_duration_scores off 47. a bool (true / false; no number, no string)
                           48. needs decode viterbi
                           49. needs a decode_duration_prior (it scores the explicit-duration grammar of that search,
                               wfl_decode_duration_posterior: the same records as decode_scores; without a prior decode_scores, or
                               bigram_scores beside a phoneme_bigram, is the option to ask for)
  transcript_variants off  50. a bool (true / false; no number, no string)
                           51. needs align viterbi (the variants are arcs of that search: the transcript graph of wfl_align_graph)
                           52. align_draft, min_duration, optional_tokens, filler_token, duration_prior, align_scores, align_edits,
                               align_insertions, duration_scores, optional_scores, filler_scores and duration_prior_scores beside
                               transcript_variants are refused, each by name (transcript_variants_error): their lattices are chains,
                               and a search or a score must speak of the lattice the search ran on -- search first, scores later
                           (53. with the model known, Labeler.label_files: an output name of the label set that holds one of `(`,
                               `|`, `)` is refused by name, align.variant_name_collisions)
"""
from __future__ import annotations

from typing import NamedTuple, Optional

from .postprocess import FRAME_DURATION

ALIGN_MODES = ("greedy", "viterbi")
DECODE_MODES = ("argmax", "viterbi")

DEFAULT_DRAFT_TOLERANCE = 0.1     # seconds; a default to start from, not a measured optimum

BIGRAM_SCORES_ERROR = ("decode_scores cannot be combined with a phoneme bigram: the forward-backward pass scores the flat switch "
                       "penalty, not the bigram the search ran on; ask for bigram_scores (postprocess.bigram_scores, --bigram-scores) "
                       "instead, which scores the bigram's own grammar")


MAX_MIN_FRAMES = 8                # the search's cap on a token's minimum duration, frames (csrc/lattice.h, align.MAX_MIN_FRAMES)
MIN_DURATION_SCORES_ERROR = ("align_scores, align_edits and align_insertions cannot be combined with a min_duration: their passes score "
                             "the lattice without minimum durations, not the one the search ran on; drop postprocess.min_duration "
                             "(--min-duration) for the scoring run")


OPTIONAL_TOKENS_ERROR = ("optional_tokens cannot be combined with min_duration, align_scores, align_edits, align_insertions or "
                         "duration_scores: their lattices have no skip arcs, and a score must speak of the lattice the search ran on; "
                         "drop postprocess.optional_tokens (--optional) for that run")


DEFAULT_FILLER_PENALTY = 1.0      # nats per frame; a value to start from, not a measured optimum
FILLER_TOKEN_ERROR = ("filler_token cannot be combined with align_draft, min_duration, optional_tokens, align_scores, align_edits, "
                      "align_insertions, duration_scores or optional_scores: their lattices have no filler emission, and a score must "
                      "speak of the lattice the search ran on; drop postprocess.filler_token (--filler-token) for that run")


FILLER_SCORES_ERROR = ("filler_scores needs a filler_token (postprocess.filler_token, --filler-token): it scores the filler lattice of "
                       "that search; without a filler_token align_scores is the option to ask for")


DEFAULT_DURATION_PRIOR_WEIGHT = 1.0   # a value to start from, not a measured optimum
DURATION_PRIOR_ERROR = ("duration_prior cannot be combined with align_draft, min_duration, optional_tokens, filler_token, align_scores, "
                        "align_edits, align_insertions, duration_scores, optional_scores or filler_scores: their lattices carry no "
                        "duration term, and a search or a score must speak of one lattice; drop postprocess.duration_prior "
                        "(--duration-prior) for that run")


DURATION_PRIOR_SCORES_ERROR = ("duration_prior_scores needs a duration_prior (postprocess.duration_prior, --duration-prior): it scores "
                               "the explicit-duration lattice of that search; without a prior align_scores is the option to ask for")


DECODE_DURATION_PRIOR_ERROR = ("decode_duration_prior cannot be combined with decode_scores or bigram_scores: their forward-backward "
                               "sweeps carry no duration term, and a posterior must score the grammar the search ran on; ask for "
                               "decode_duration_scores (postprocess.decode_duration_scores, --decode-duration-scores) instead, which "
                               "scores the explicit-duration grammar of that search")


DECODE_DURATION_SCORES_ERROR = ("decode_duration_scores needs a decode_duration_prior (postprocess.decode_duration_prior, "
                                "--decode-duration-prior): it scores the explicit-duration grammar of that search; without a prior "
                                "decode_scores (or bigram_scores beside a phoneme_bigram) is the option to ask for")


# the options whose lattices are chains: refused beside transcript_variants, each by name
CHAIN_ONLY_OPTIONS = ("align_draft", "min_duration", "optional_tokens", "filler_token", "duration_prior", "align_scores", "align_edits",
                      "align_insertions", "duration_scores", "optional_scores", "filler_scores", "duration_prior_scores")


def transcript_variants_error(names):
    return (f"transcript_variants cannot be combined with {', '.join(names)}: their lattices are chains, the variants' is a graph, and "
            "a search or a score must speak of the lattice the search ran on; drop postprocess.transcript_variants "
            "(--transcript-variants) for that run, or search with the variants first and score the chosen transcript later")


def _filler_token(given):
    """postprocess.filler_token -> None (absent) or the name; anything but a non-empty string without whitespace breaks rule 27."""
    if given is None:
        return None
    if isinstance(given, str) and given and not any(ch.isspace() for ch in given):
        return given
    raise ValueError(f"filler_token must be a non-empty string without whitespace, got {given!r}")


def filler_token_collision(filler_token, output_names):
    """Rule 32, for the caller that knows the model: the filler_token when it is an output name of the label set, else None."""
    return filler_token if filler_token is not None and filler_token in set(output_names) else None


def _optional_tokens(given):
    """postprocess.optional_tokens -> its normalised, hashable form: None (absent, or an empty list), "*" (every token), or a sorted
    tuple of distinct names.  Anything else breaks rule 19."""
    if given is None:
        return None
    if isinstance(given, str):
        if given == "*":
            return "*"
    elif isinstance(given, (list, tuple, set, frozenset)) and all(isinstance(x, str) and x for x in given):
        return ("*" if "*" in given else tuple(sorted(set(given)))) or None
    raise ValueError(f"optional_tokens must be a list of token names or '*', got {given!r}")


def unknown_optional_tokens(optional_tokens, output_names):
    """Rule 24, for the caller that knows the model: the names of `optional_tokens` that are no output name of the label set."""
    if optional_tokens in (None, "*"):
        return []
    known = set(output_names)
    return [n for n in optional_tokens if n not in known]


def _min_duration(given):
    """postprocess.min_duration -> its normalised, hashable form: None (absent, or an empty mapping), a float (one value for every
    token), or a tuple of (name, seconds) pairs sorted by name ("default" among them) -- dict() of it is the mapping again.  A value
    that breaks rule 14 is a ValueError.  An iterable of pairs (the normalised form itself) is taken as a mapping."""
    limit = MAX_MIN_FRAMES * FRAME_DURATION

    def seconds(x):
        v = _number_ge0(x)
        if v is None or v > limit + 1e-9:
            raise ValueError(f"min_duration must be a number of seconds between 0 and {limit:g} ({MAX_MIN_FRAMES} frames), or a mapping "
                             f"of token names (and 'default') to such numbers, got {x!r}")
        return v
    if given is None:
        return None
    if isinstance(given, (tuple, list)):
        try:
            given = dict(given)
        except (TypeError, ValueError):
            seconds(given)
    if isinstance(given, dict):
        return tuple(sorted((str(k), seconds(v)) for k, v in given.items())) or None
    return seconds(given)


def parse_min_duration(values):
    """The CLI's repeatable --min-duration values, each SECONDS or NAME=SECONDS -> what `resolve` takes: None (no value), a float (one
    plain SECONDS) or a mapping, a plain SECONDS among named ones being its "default".  A SECONDS that is no number stays a string
    for rule 14 to report."""
    def num(x):
        try:
            return float(x)
        except ValueError:
            return x
    values = list(values or ())
    if not values:
        return None
    if len(values) == 1 and "=" not in values[0]:
        return num(values[0])
    out = {}
    for v in values:
        name, eq, sec = v.rpartition("=")
        out[name if eq else "default"] = num(sec)
    return out


class _SearchOptions(NamedTuple):
    align: str = "greedy"
    align_scores: bool = False
    decode: str = "argmax"
    switch_penalty: float = 0.0               # nats per opened run (decode viterbi)
    decode_scores: bool = False
    phoneme_bigram: Optional[str] = None      # path of a phoneme_bigram.json; an empty path is None
    bigram_weight: float = 1.0                # (1.0 also stands for "not given")
    bigram_scores: bool = False

    @property
    def free_scores(self) -> bool:
        """Scores of the grammar search's path are asked for, of either kind."""
        return self.decode_scores or self.bigram_scores

    @property
    def scored(self) -> bool:
        return self.align_scores or self.free_scores


class PostOptions(_SearchOptions):
    """The record `resolve` returns.  The eight options of the searches are the tuple (positional, `_fields`, as they have been);
    the later ones follow them as keyword fields with defaults, read-only like the rest and part of equality, hash and repr:

        align_draft      None   folder of draft .lab files (X.wav -> DIR/X.lab); an empty path is None
        draft_tolerance  0.1    seconds either side of a draft start (also stands for "not given")
        align_edits      False  score single substitutions and deletions of every aligned transcript
        align_insertions False  score single insertions at every place of every aligned transcript
        min_duration     None   the least time a transcript token occupies: seconds, or ((name, seconds), ...) sorted by name
        duration_scores  False  score every alignment searched under a min_duration, over the minimum-duration lattice
        optional_tokens  None   the tokens a path may leave out: "*", or a sorted tuple of names
        skip_penalty     0.0    nats a path pays per skipped token (also stands for "not given")
        optional_scores  False  score every alignment searched with optional_tokens, over the skip lattice
        filler_token     None   the transcript token that matches anything
        filler_penalty   1.0    nats a filler pays per frame of its run (also stands for "not given")
        filler_scores    False  score every alignment searched with a filler_token, over the filler lattice
        duration_prior   None   path of a phoneme_durations.json: the duration prior of the explicit-duration search
        duration_prior_weight  1.0  what the prior's log probabilities are multiplied by (also stands for "not given")
        duration_prior_scores  False  score every alignment searched under a duration_prior, over the explicit-duration lattice
        decode_duration_prior  None  path of a phoneme_durations.json: the duration prior of the free decode (decode viterbi)
        decode_duration_prior_weight  1.0  what that prior's log probabilities are multiplied by (also stands for "not given")
        decode_duration_scores  False  score every file decoded under a decode_duration_prior, over the explicit-duration grammar
        transcript_variants  False  `( a | b )` groups of a transcript are variants the search chooses among (wfl_align_graph)"""
    align_draft: Optional[str] = None
    draft_tolerance: float = DEFAULT_DRAFT_TOLERANCE
    align_edits: bool = False
    align_insertions: bool = False
    min_duration: object = None
    duration_scores: bool = False
    optional_tokens: object = None
    skip_penalty: float = 0.0
    optional_scores: bool = False
    filler_token: Optional[str] = None
    filler_penalty: float = DEFAULT_FILLER_PENALTY
    filler_scores: bool = False
    duration_prior: Optional[str] = None
    duration_prior_weight: float = DEFAULT_DURATION_PRIOR_WEIGHT
    duration_prior_scores: bool = False
    decode_duration_prior: Optional[str] = None
    decode_duration_prior_weight: float = DEFAULT_DURATION_PRIOR_WEIGHT
    decode_duration_scores: bool = False
    transcript_variants: bool = False

    def __new__(cls, *args, align_draft=None, draft_tolerance=DEFAULT_DRAFT_TOLERANCE, align_edits=False, align_insertions=False,
                min_duration=None, duration_scores=False, optional_tokens=None, skip_penalty=0.0, optional_scores=False,
                filler_token=None, filler_penalty=DEFAULT_FILLER_PENALTY, filler_scores=False, duration_prior=None,
                duration_prior_weight=DEFAULT_DURATION_PRIOR_WEIGHT, duration_prior_scores=False, decode_duration_prior=None,
                decode_duration_prior_weight=DEFAULT_DURATION_PRIOR_WEIGHT, decode_duration_scores=False, transcript_variants=False, **kw):
        self = super().__new__(cls, *args, **kw)
        object.__setattr__(self, "align_draft", align_draft)
        object.__setattr__(self, "draft_tolerance", draft_tolerance)
        object.__setattr__(self, "align_edits", align_edits)
        object.__setattr__(self, "align_insertions", align_insertions)
        object.__setattr__(self, "min_duration", min_duration)
        object.__setattr__(self, "duration_scores", duration_scores)
        object.__setattr__(self, "optional_tokens", optional_tokens)
        object.__setattr__(self, "skip_penalty", skip_penalty)
        object.__setattr__(self, "optional_scores", optional_scores)
        object.__setattr__(self, "filler_token", filler_token)
        object.__setattr__(self, "filler_penalty", filler_penalty)
        object.__setattr__(self, "filler_scores", filler_scores)
        object.__setattr__(self, "duration_prior", duration_prior)
        object.__setattr__(self, "duration_prior_weight", duration_prior_weight)
        object.__setattr__(self, "duration_prior_scores", duration_prior_scores)
        object.__setattr__(self, "decode_duration_prior", decode_duration_prior)
        object.__setattr__(self, "decode_duration_prior_weight", decode_duration_prior_weight)
        object.__setattr__(self, "decode_duration_scores", decode_duration_scores)
        object.__setattr__(self, "transcript_variants", transcript_variants)
        return self

    def __setattr__(self, name, value):
        raise AttributeError(f"PostOptions is read-only: cannot set {name!r}")

    _KEYWORD = ("align_draft", "draft_tolerance", "align_edits", "align_insertions", "min_duration", "duration_scores",
                "optional_tokens", "skip_penalty", "duration_prior", "duration_prior_weight", "decode_duration_prior",
                "decode_duration_prior_weight", "decode_duration_scores", "transcript_variants", "filler_scores", "duration_prior_scores", "optional_scores", "filler_token", "filler_penalty")
    # (the later options stand in front of optional_scores: the record's last fields are the filler's own two)
    _KEYWORD_DEFAULTS = (None, DEFAULT_DRAFT_TOLERANCE, False, False, None, False, None, 0.0, None, DEFAULT_DURATION_PRIOR_WEIGHT,
                         None, DEFAULT_DURATION_PRIOR_WEIGHT, False, False, False, False, False, None, DEFAULT_FILLER_PENALTY)

    def _draft(self):
        return self.align_draft, self.draft_tolerance

    @property
    def free_scores(self) -> bool:
        """Scores of the grammar search's path are asked for, of any of the three kinds."""
        return self.decode_scores or self.bigram_scores or self.decode_duration_scores

    @property
    def scored(self) -> bool:
        return (self.align_scores or self.free_scores or self.duration_scores or self.optional_scores or self.filler_scores
                or self.duration_prior_scores)

    def _later(self):
        return tuple(getattr(self, k) for k in self._KEYWORD)

    # the NamedTuple helpers carry the keyword fields as well (the inherited ones know the tuple alone)
    @classmethod
    def _make(cls, iterable, align_draft=None, draft_tolerance=DEFAULT_DRAFT_TOLERANCE, align_edits=False, align_insertions=False,
              min_duration=None, duration_scores=False, optional_tokens=None, skip_penalty=0.0, optional_scores=False,
              filler_token=None, filler_penalty=DEFAULT_FILLER_PENALTY, filler_scores=False, duration_prior=None,
              duration_prior_weight=DEFAULT_DURATION_PRIOR_WEIGHT, duration_prior_scores=False, decode_duration_prior=None,
              decode_duration_prior_weight=DEFAULT_DURATION_PRIOR_WEIGHT, decode_duration_scores=False, transcript_variants=False):
        return cls(*iterable, align_draft=align_draft, draft_tolerance=draft_tolerance, align_edits=align_edits,
                   align_insertions=align_insertions, min_duration=min_duration, duration_scores=duration_scores,
                   optional_tokens=optional_tokens, skip_penalty=skip_penalty, optional_scores=optional_scores,
                   filler_token=filler_token, filler_penalty=filler_penalty, filler_scores=filler_scores,
                   duration_prior=duration_prior, duration_prior_weight=duration_prior_weight,
                   duration_prior_scores=duration_prior_scores, decode_duration_prior=decode_duration_prior,
                   decode_duration_prior_weight=decode_duration_prior_weight, decode_duration_scores=decode_duration_scores,
                   transcript_variants=transcript_variants)

    def _replace(self, **kw):
        later = {k: kw.pop(k, getattr(self, k)) for k in self._KEYWORD}
        return type(self)(*super()._replace(**kw), **later)

    def _asdict(self):
        return {**super()._asdict(), **{k: getattr(self, k) for k in self._KEYWORD}}

    def __eq__(self, other):
        """Equal to another PostOptions with the same values; to a plain tuple of the eight only while the keyword fields are at
        their defaults (where a PostOptions of those eight would be equal, too)."""
        theirs = other._later() if isinstance(other, PostOptions) else self._KEYWORD_DEFAULTS
        return tuple.__eq__(self, other) is True and self._later() == theirs

    def __ne__(self, other):
        return not self == other

    def __hash__(self):     # (equal to a plain tuple only with the default keyword fields: then the tuple's own hash)
        return tuple.__hash__(self) if self._later() == self._KEYWORD_DEFAULTS else hash((tuple(self), self._later()))

    def __repr__(self):
        return super().__repr__()[:-1] + "".join(f", {k}={getattr(self, k)!r}" for k in self._KEYWORD) + ")"


def _number_ge0(x):
    """float(x) for a number >= 0; None for anything else (a bool, a NaN, a negative, a string that is no number)."""
    try:
        v = float(x)
    except (TypeError, ValueError):
        return None
    return v if v >= 0.0 and not isinstance(x, bool) else None


def resolve(post, *, align=None, align_scores=None, decode=None, switch_penalty=None, decode_scores=None, phoneme_bigram=None,
            bigram_weight=None, bigram_scores=None, decode_duration_prior=None, decode_duration_prior_weight=None, decode_duration_scores=None,
            transcript_variants=None, align_draft=None, draft_tolerance=None, align_edits=None,
            align_insertions=None, min_duration=None, duration_scores=None, optional_tokens=None, skip_penalty=None,
            optional_scores=None, filler_token=None, filler_penalty=None, filler_scores=None, duration_prior=None,
            duration_prior_weight=None, duration_prior_scores=None) -> PostOptions:
    """post: the config's `postprocess` mapping (None: {}).  Per option the argument wins; None leaves it to `post[<option>]`, and a
    key that is absent (or None) to the default.  -> PostOptions, or ValueError for the first broken rule of the module's table."""
    post = post or {}

    def pick(key, arg, default=None):
        if arg is None:
            arg = post.get(key)
        return default if arg is None else arg

    align = pick("align", align, "greedy")
    if align not in ALIGN_MODES:
        raise ValueError(f"align must be one of {ALIGN_MODES}, got {align!r}")
    align_scores = bool(pick("align_scores", align_scores, False))
    if align_scores and align != "viterbi":
        raise ValueError("align_scores needs align='viterbi' (postprocess.align: viterbi): the greedy match has no lattice to score")
    decode = pick("decode", decode, "argmax")
    if decode not in DECODE_MODES:
        raise ValueError(f"decode must be one of {DECODE_MODES}, got {decode!r}")
    given = pick("switch_penalty", switch_penalty, 0.0)
    switch_penalty = _number_ge0(given)
    if switch_penalty is None:
        raise ValueError(f"switch_penalty must be a number >= 0 (nats), got {given!r}")
    decode_scores = bool(pick("decode_scores", decode_scores, False))
    if decode_scores and decode != "viterbi":
        raise ValueError("decode_scores needs decode='viterbi' (postprocess.decode: viterbi): the argmax decode has no lattice to score")
    given = pick("bigram_weight", bigram_weight)
    bigram_weight = 1.0 if given is None else _number_ge0(given)
    if bigram_weight is None:
        raise ValueError(f"bigram_weight must be a number >= 0, got {given!r}")
    phoneme_bigram = pick("phoneme_bigram", phoneme_bigram)
    phoneme_bigram = str(phoneme_bigram) if phoneme_bigram else None
    if (phoneme_bigram or given is not None) and decode != "viterbi":
        raise ValueError("phoneme_bigram / bigram_weight need decode='viterbi' (postprocess.decode: viterbi): the argmax decode has no "
                         "search to weigh")
    if phoneme_bigram and decode_scores:
        raise ValueError(BIGRAM_SCORES_ERROR)
    bigram_scores = bool(pick("bigram_scores", bigram_scores, False))
    if bigram_scores and decode != "viterbi":
        raise ValueError("bigram_scores needs decode='viterbi' (postprocess.decode: viterbi) and a phoneme_bigram: the argmax decode "
                         "has no lattice to score")
    if bigram_scores and not phoneme_bigram:
        raise ValueError("bigram_scores needs a phoneme_bigram (postprocess.phoneme_bigram): it scores the bigram search's path; "
                         "decode_scores scores a search under the flat switch penalty")
    align_draft = pick("align_draft", align_draft)
    align_draft = str(align_draft) if align_draft else None
    if align_draft and align != "viterbi":
        raise ValueError("align_draft needs align='viterbi' (postprocess.align: viterbi): the draft's windows hold the Viterbi search, "
                         "the greedy match has none")
    given = pick("draft_tolerance", draft_tolerance)
    draft_tolerance = DEFAULT_DRAFT_TOLERANCE if given is None else _number_ge0(given)
    if draft_tolerance is None:
        raise ValueError(f"draft_tolerance must be a number >= 0 (seconds), got {given!r}")
    if given is not None and not align_draft:
        raise ValueError("draft_tolerance needs an align_draft (postprocess.align_draft): it is the half-width of the draft's windows")
    align_edits = bool(pick("align_edits", align_edits, False))
    if align_edits and align != "viterbi":
        raise ValueError("align_edits needs align='viterbi' (postprocess.align: viterbi): the greedy match has no lattice to score an "
                         "edit on")
    align_insertions = bool(pick("align_insertions", align_insertions, False))
    if align_insertions and align != "viterbi":
        raise ValueError("align_insertions needs align='viterbi' (postprocess.align: viterbi): the greedy match has no lattice to "
                         "score an insertion on")
    min_duration = _min_duration(pick("min_duration", min_duration))
    if min_duration is not None and align != "viterbi":
        raise ValueError("min_duration needs align='viterbi' (postprocess.align: viterbi): the durations constrain the Viterbi search, "
                         "the greedy match has none")
    if min_duration is not None and (align_scores or align_edits or align_insertions):
        raise ValueError(MIN_DURATION_SCORES_ERROR)
    duration_scores = bool(pick("duration_scores", duration_scores, False))
    if duration_scores and align != "viterbi":
        raise ValueError("duration_scores needs align='viterbi' (postprocess.align: viterbi) and a min_duration: the greedy match has "
                         "no lattice to score")
    if duration_scores and min_duration is None:
        raise ValueError("duration_scores needs a min_duration (postprocess.min_duration): it scores the minimum-duration lattice of "
                         "that search; without durations align_scores is the option to ask for")
    optional_tokens = _optional_tokens(pick("optional_tokens", optional_tokens))
    if optional_tokens is not None and align != "viterbi":
        raise ValueError("optional_tokens needs align='viterbi' (postprocess.align: viterbi): the skip arcs are arcs of the Viterbi "
                         "search, the greedy match has none")
    given = pick("skip_penalty", skip_penalty)
    skip_penalty = 0.0 if given is None else _number_ge0(given)
    if skip_penalty is None or skip_penalty == float("inf"):
        raise ValueError(f"skip_penalty must be a number >= 0 (nats per skipped token), got {given!r}")
    if given is not None and optional_tokens is None:
        raise ValueError("skip_penalty needs optional_tokens (postprocess.optional_tokens): it is the price of skipping one of them")
    if optional_tokens is not None and (min_duration is not None or align_scores or align_edits or align_insertions or duration_scores):
        raise ValueError(OPTIONAL_TOKENS_ERROR)
    optional_scores = bool(pick("optional_scores", optional_scores, False))
    if optional_scores and align != "viterbi":
        raise ValueError("optional_scores needs align='viterbi' (postprocess.align: viterbi) and optional_tokens: the greedy match has "
                         "no lattice to score")
    if optional_scores and optional_tokens is None:
        raise ValueError("optional_scores needs optional_tokens (postprocess.optional_tokens): it scores the skip lattice of that "
                         "search; without optional tokens align_scores is the option to ask for")
    filler_token = _filler_token(pick("filler_token", filler_token))
    if filler_token is not None and align != "viterbi":
        raise ValueError("filler_token needs align='viterbi' (postprocess.align: viterbi): the filler is a token of the Viterbi search, "
                         "the greedy match has none")
    given = pick("filler_penalty", filler_penalty)
    filler_penalty = DEFAULT_FILLER_PENALTY if given is None else _number_ge0(given)
    if filler_penalty is None or filler_penalty == float("inf"):
        raise ValueError(f"filler_penalty must be a finite number >= 0 (nats per frame of a filler), got {given!r}")
    if given is not None and filler_token is None:
        raise ValueError("filler_penalty needs a filler_token (postprocess.filler_token): it is the price per frame of that token")
    if filler_token is not None and (align_draft or min_duration is not None or optional_tokens is not None or align_scores or align_edits
                                     or align_insertions or duration_scores or optional_scores):
        raise ValueError(FILLER_TOKEN_ERROR)
    filler_scores = pick("filler_scores", filler_scores, False)
    if not isinstance(filler_scores, bool):
        raise ValueError(f"filler_scores must be true or false, got {filler_scores!r}")
    if filler_scores and filler_token is None:
        raise ValueError(FILLER_SCORES_ERROR)
    duration_prior = pick("duration_prior", duration_prior)
    duration_prior = str(duration_prior) if duration_prior else None
    if duration_prior and align != "viterbi":
        raise ValueError("duration_prior needs align='viterbi' (postprocess.align: viterbi): the prior is a term of the Viterbi search's "
                         "path score, the greedy match has none")
    given = pick("duration_prior_weight", duration_prior_weight)
    duration_prior_weight = DEFAULT_DURATION_PRIOR_WEIGHT if given is None else _number_ge0(given)
    if duration_prior_weight is None or duration_prior_weight == float("inf"):
        raise ValueError(f"duration_prior_weight must be a finite number >= 0, got {given!r}")
    if given is not None and not duration_prior:
        raise ValueError("duration_prior_weight needs a duration_prior (postprocess.duration_prior): it scales that prior")
    if duration_prior and (align_draft or min_duration is not None or optional_tokens is not None or filler_token is not None
                           or align_scores or align_edits or align_insertions or duration_scores or optional_scores or filler_scores):
        raise ValueError(DURATION_PRIOR_ERROR)
    duration_prior_scores = pick("duration_prior_scores", duration_prior_scores, False)
    if not isinstance(duration_prior_scores, bool):
        raise ValueError(f"duration_prior_scores must be true or false, got {duration_prior_scores!r}")
    if duration_prior_scores and not duration_prior:
        raise ValueError(DURATION_PRIOR_SCORES_ERROR)
    decode_duration_prior = pick("decode_duration_prior", decode_duration_prior)
    decode_duration_prior = str(decode_duration_prior) if decode_duration_prior else None
    given = pick("decode_duration_prior_weight", decode_duration_prior_weight)
    if (decode_duration_prior or given is not None) and decode != "viterbi":
        raise ValueError("decode_duration_prior / decode_duration_prior_weight need decode='viterbi' (postprocess.decode: viterbi): the "
                         "argmax decode has no search to weigh")
    decode_duration_prior_weight = DEFAULT_DURATION_PRIOR_WEIGHT if given is None else _number_ge0(given)
    if decode_duration_prior_weight is None or decode_duration_prior_weight == float("inf"):
        raise ValueError(f"decode_duration_prior_weight must be a finite number >= 0, got {given!r}")
    if given is not None and not decode_duration_prior:
        raise ValueError("decode_duration_prior_weight needs a decode_duration_prior (postprocess.decode_duration_prior): it scales that "
                         "prior")
    if decode_duration_prior and (decode_scores or bigram_scores):
        raise ValueError(DECODE_DURATION_PRIOR_ERROR)
    decode_duration_scores = pick("decode_duration_scores", decode_duration_scores, False)
    if not isinstance(decode_duration_scores, bool):
        raise ValueError(f"decode_duration_scores must be true or false, got {decode_duration_scores!r}")
    if decode_duration_scores and decode != "viterbi":
        raise ValueError("decode_duration_scores needs decode='viterbi' (postprocess.decode: viterbi) and a decode_duration_prior: the "
                         "argmax decode has no lattice to score")
    if decode_duration_scores and not decode_duration_prior:
        raise ValueError(DECODE_DURATION_SCORES_ERROR)
    transcript_variants = pick("transcript_variants", transcript_variants, False)
    if not isinstance(transcript_variants, bool):
        raise ValueError(f"transcript_variants must be true or false, got {transcript_variants!r}")
    if transcript_variants and align != "viterbi":
        raise ValueError("transcript_variants needs align='viterbi' (postprocess.align: viterbi): the variants are arcs of the Viterbi "
                         "search, the greedy match has none")
    if transcript_variants:
        given = {"align_draft": align_draft, "min_duration": min_duration is not None, "optional_tokens": optional_tokens is not None,
                 "filler_token": filler_token is not None, "duration_prior": duration_prior, "align_scores": align_scores,
                 "align_edits": align_edits, "align_insertions": align_insertions, "duration_scores": duration_scores,
                 "optional_scores": optional_scores, "filler_scores": filler_scores, "duration_prior_scores": duration_prior_scores}
        beside = [k for k in CHAIN_ONLY_OPTIONS if given[k]]
        if beside:
            raise ValueError(transcript_variants_error(beside))
    return PostOptions(align, align_scores, decode, switch_penalty, decode_scores, phoneme_bigram, bigram_weight, bigram_scores,
                       align_draft=align_draft, draft_tolerance=draft_tolerance, align_edits=align_edits,
                       align_insertions=align_insertions, min_duration=min_duration, duration_scores=duration_scores,
                       optional_tokens=optional_tokens, skip_penalty=skip_penalty, optional_scores=optional_scores,
                       filler_token=filler_token, filler_penalty=filler_penalty, filler_scores=filler_scores,
                       duration_prior=duration_prior, duration_prior_weight=duration_prior_weight,
                       duration_prior_scores=duration_prior_scores, decode_duration_prior=decode_duration_prior,
                       decode_duration_prior_weight=decode_duration_prior_weight, decode_duration_scores=decode_duration_scores,
                       transcript_variants=transcript_variants)
