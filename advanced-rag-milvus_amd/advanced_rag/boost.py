"""Boost ranker and function score: final = normalised relevance (x or +) the combined weight of the filter expressions a
row matches, then a stable sort.

The contract is the table in include/hbmrag.h (hr_boost_rerank_dev).  This module holds the spec objects a caller passes
(`BoostRanker` and its container `FunctionScore`, named after pymilvus' rankers of the same purpose) and the pure-Python
restatement of the device kernel (csrc/boost.h): every operation one IEEE fp64 operation on Python floats, the draw an
integer mix on Python ints, so that host and device agree bit for bit."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Any, List, Optional, Sequence, Tuple

from ._native import (HR_BOOST_MULTIPLY, HR_BOOST_SUM, HR_MAX_BOOST_FUNCS, HR_NORM_MINMAX, HR_NORM_MINMAX_DIST,
                      HR_NORM_NONE)   # importing the binding module does not load the library

BOOST_MODES = {"multiply": HR_BOOST_MULTIPLY, "sum": HR_BOOST_SUM}
BOOST_NORMALIZATIONS = ("none", "activation", "minmax")
# what a draw may be keyed by: the int64 group keys PayloadColumns.group_keys / DeviceGroupKeys hold ("chunk_id" = "id")
BOOST_KEY_FIELDS = ("doc_id", "id", "chunk_id", "timestamp", "chunk_index", "token_count")

_M64 = (1 << 64) - 1
_GOLDEN = 0x9E3779B97F4A7C15


def _mix(z: int) -> int:
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & _M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def canonical_random(seed: int, key: int) -> float:
    """The draw of the boost ranker, u in [0, 1): the splitmix64 finaliser over the seed, then over the key (an int64,
    taken mod 2^64), the top 53 bits as an exact double.  The same bits as csrc/boost.h."""
    h = _mix((int(seed) + _GOLDEN) & _M64)
    z = _mix(((h ^ (int(key) & _M64)) + _GOLDEN) & _M64)
    return float(z >> 11) * 2.0 ** -53


def _mode(name: str, value: Any) -> int:
    if isinstance(value, str) and value in BOOST_MODES:
        return BOOST_MODES[value]
    if not isinstance(value, bool) and isinstance(value, int) and value in (HR_BOOST_MULTIPLY, HR_BOOST_SUM):
        return int(value)
    raise ValueError(f"{name} must be one of {', '.join(BOOST_MODES)}, got {value!r}")


@dataclass(frozen=True)
class BoostRanker:
    """One function of a function score; passed alone as a ranker it is FunctionScore(it).

    filter        an expression of the filter language (`in` lists, TEXT_MATCH, ...): the rows the function matches;
                  None matches every row
    weight        the function's value for a matching row: a finite number (below 1 demotes under "multiply")
    random_score  None, or {"seed": int in [0, 2^64), "field": None | a group-key field}: the value becomes weight * u,
                  u in [0, 1) drawn from (seed, the row's key of `field`) — doc_id gives all chunks of a document one
                  draw.  field=None keys the draw by the global row number, which compact() renumbers: name a field for a
                  draw that survives compaction.
    """
    filter: Optional[str] = None
    weight: float = 1.0
    random_score: Optional[dict] = None

    def __post_init__(self):
        if self.filter is not None and (not isinstance(self.filter, str) or not self.filter.strip()):
            raise ValueError(f"filter must be a filter expression or None, got {self.filter!r}")
        w = self.weight
        if isinstance(w, bool) or not isinstance(w, (int, float)) or not math.isfinite(float(w)):
            raise ValueError(f"weight must be a finite number, got {w!r}")
        rs = self.random_score
        if rs is not None:
            if not isinstance(rs, dict) or not set(rs) <= {"seed", "field"} or "seed" not in rs:
                raise ValueError(f"random_score must be None or {{'seed': int, 'field': name or None}}, got {rs!r}")
            seed, field = rs["seed"], rs.get("field")
            if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed <= _M64:
                raise ValueError(f"random_score seed must be an integer in [0, 2^64), got {seed!r}")
            if field is not None and (not isinstance(field, str) or field not in BOOST_KEY_FIELDS):
                raise ValueError(f"random_score field must be None or one of {', '.join(BOOST_KEY_FIELDS)}, got {field!r}")

    @property
    def seed(self) -> Optional[int]:
        return None if self.random_score is None else int(self.random_score["seed"])

    @property
    def field(self) -> Optional[str]:
        return None if self.random_score is None else self.random_score.get("field")

    def operands(self) -> Tuple[Optional[str], float, Optional[int], Optional[str]]:
        """(filter, weight, seed or None, key field or None): what a request carries for this function."""
        return (self.filter, float(self.weight), self.seed, self.field)


class FunctionScore:
    """search(..., ranker=FunctionScore(...)) / RetrievalConfig(boost=FunctionScore(...)): 1..8 BoostRankers.

    function_mode  how the values of the matching functions combine, in the order given: "multiply" or "sum"
    boost_mode     how the combined value meets the relevance: "multiply" or "sum"; a row no function matches keeps its
                   relevance as it is
    normalization  what the relevance is: "none" (the raw score), "activation" (by the collection's metric) or "minmax".
                   With "none" on an L2 collection the raw DISTANCE is boosted and the list is sorted ascending (a weight
                   below 1 promotes, as in Milvus); the other two map distances to similarities and sort descending.
    candidates     rerank the best max(top_k, candidates) rows of the plain ranking instead of the best top_k
    """

    def __init__(self, *functions: BoostRanker, function_mode: str = "multiply", boost_mode: str = "multiply",
                 normalization: str = "none", candidates: Optional[int] = None):
        if not 1 <= len(functions) <= HR_MAX_BOOST_FUNCS:
            raise ValueError(f"functions: 1 to HR_MAX_BOOST_FUNCS = {HR_MAX_BOOST_FUNCS} BoostRankers, got {len(functions)}")
        for f in functions:
            if not isinstance(f, BoostRanker):
                raise ValueError(f"functions must be BoostRankers, got {f!r}")
        if not isinstance(normalization, str) or normalization not in BOOST_NORMALIZATIONS:
            raise ValueError(f"normalization must be one of {', '.join(BOOST_NORMALIZATIONS)}, got {normalization!r}")
        if candidates is not None and (isinstance(candidates, bool) or not isinstance(candidates, int) or candidates < 1):
            raise ValueError(f"candidates must be an integer >= 1 or None, got {candidates!r}")
        self.function_code = _mode("function_mode", function_mode)
        self.boost_code = _mode("boost_mode", boost_mode)
        self.functions = tuple(functions)
        self.function_mode, self.boost_mode = function_mode, boost_mode
        self.normalization, self.candidates = normalization, candidates

    def __repr__(self):
        return (f"FunctionScore({', '.join(map(repr, self.functions))}, function_mode={self.function_mode!r}, "
                f"boost_mode={self.boost_mode!r}, normalization={self.normalization!r}, candidates={self.candidates!r})")

    @staticmethod
    def of(ranker: Any, name: str = "ranker") -> "FunctionScore":
        """A FunctionScore as it is, a bare BoostRanker as FunctionScore(it); ValueError for anything else."""
        if isinstance(ranker, FunctionScore):
            return ranker
        if isinstance(ranker, BoostRanker):
            return FunctionScore(ranker)
        raise ValueError(f"{name} must be a FunctionScore or a BoostRanker, got {ranker!r}")

    def window(self, top_k: int) -> int:
        """W: how deep the plain ranking is read before the rerank."""
        return max(int(top_k), int(self.candidates or top_k))

    def operands(self) -> Tuple[Tuple, ...]:
        return tuple(f.operands() for f in self.functions)

    def ascending(self, metric: str, fused: bool = False) -> bool:
        """The list is sorted ascending: raw distances of an L2 collection."""
        return not fused and self.normalization == "none" and str(metric).upper() == "L2"

    def norm_code(self, metric: str, fused: bool = False) -> int:
        """HR_NORM_* (or HR_NORM_NONE) for a list ranked by `metric`.  fused = the list holds RRF / weighted fused scores,
        which are not renormalised: "activation" means identity there."""
        if self.normalization == "minmax":
            return HR_NORM_MINMAX_DIST if not fused and str(metric).upper() == "L2" else HR_NORM_MINMAX
        if fused or self.normalization == "none":
            return HR_NORM_NONE
        from .retrieval import norm_code
        return norm_code(metric, "activation")

    def launch_key(self, metric: str, fused: bool = False) -> Tuple[int, int, int, int]:
        """(function mode, boost mode, norm code, direction): what requests must share to share a launch."""
        return (self.function_code, self.boost_code, self.norm_code(metric, fused), int(self.ascending(metric, fused)))


def normalise(scores: Sequence[float], code: int) -> List[float]:
    """n(s) of the table for scores that are already doubles: decay.normalise."""
    from .decay import normalise as _normalise
    return _normalise(scores, code)


def _sort_key(ascending: bool):
    # a NaN after every number in either direction; -v is exact, and -0.0 == 0.0 stays one tie
    return lambda fv: (1, 0.0) if fv != fv else (0, fv if ascending else -fv)


def boost_rerank(ids: Sequence[int], scores: Sequence[float], matches: Sequence[Sequence[bool]],
                 values_or_specs: Sequence[Any], function_mode: Any = 0, boost_mode: Any = 0, norm: int = HR_NORM_NONE,
                 ascending: bool = False, k_out: Optional[int] = None
                 ) -> Tuple[List[int], List[int], List[float], List[int]]:
    """Host restatement of hr_boost_rerank_dev for ONE list: ids / scores = the list's valid prefix (scores as doubles:
    fp32 scores widened, or fp64), matches[j][i] = function j matches entry i (all False for an inactive slot),
    values_or_specs[j] = the function's weight, or (weight, seed, keys) for a draw with keys[i] the key of entry i (the
    key column's value, or the id where the column does not cover the row).
    -> (positions, ids, final scores, matched bits) of the first k_out entries in the stable order of final; shorter
    than k_out when the list is (the device pads with -1 / -1 / 0.0 / 0)."""
    n = len(ids)
    fmode, bmode = _mode("function_mode", function_mode), _mode("boost_mode", boost_mode)
    if len(matches) != len(values_or_specs) or not 1 <= len(matches) <= HR_MAX_BOOST_FUNCS:
        raise ValueError(f"1 to {HR_MAX_BOOST_FUNCS} functions with one value each, got {len(matches)} / {len(values_or_specs)}")
    ns = normalise(scores, norm)
    final, bits = [], []
    for i in range(n):
        f, matched = 0.0, 0
        for j, spec in enumerate(values_or_specs):
            if not matches[j][i]:
                continue
            if isinstance(spec, (tuple, list)):
                weight, seed, keys = spec
                v = float(weight) * canonical_random(seed, keys[i])
            else:
                v = float(spec)
            f = v if not matched else (f + v if fmode == HR_BOOST_SUM else f * v)
            matched |= 1 << j
        final.append(ns[i] if not matched else (ns[i] + f if bmode == HR_BOOST_SUM else ns[i] * f))
        bits.append(matched)
    key = _sort_key(bool(ascending))
    order = sorted(range(n), key=lambda i: key(final[i]))[:n if k_out is None else k_out]   # stable: ties keep input order
    return order, [ids[i] for i in order], [final[i] for i in order], [bits[i] for i in order]


def matched_functions(bits: int) -> List[int]:
    """The function indices of a matched-bits word, ascending: a hit's "boosted_by"."""
    return [j for j in range(HR_MAX_BOOST_FUNCS) if (int(bits) >> j) & 1]
