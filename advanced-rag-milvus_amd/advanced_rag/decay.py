"""Decay ranker: final = normalised relevance x decay(|field - origin|), then a stable descending sort.

The contract is the table in include/hbmrag.h (hr_decay_rerank_dev).  This module holds the spec object a caller passes
(`DecayRanker`, named after pymilvus' ranker of the same purpose) and the pure-Python restatement of the device kernel
(csrc/decay.h): every operation one IEEE fp64 operation on Python floats, so that host and device agree bit for bit."""
from __future__ import annotations

import math
import time
from dataclasses import dataclass
from datetime import datetime, timezone
from typing import Any, List, Optional, Sequence, Tuple

from ._native import (HR_DECAY_EXP, HR_DECAY_GAUSS, HR_DECAY_LINEAR, HR_NORM_MINMAX, HR_NORM_MINMAX_DIST,
                      HR_NORM_NONE)   # importing the binding module does not load the library

DECAY_FUNCTIONS = {"gauss": HR_DECAY_GAUSS, "exp": HR_DECAY_EXP, "linear": HR_DECAY_LINEAR}
DECAY_NORMALIZATIONS = ("activation", "minmax", "none")
# field -> how the column is held: "epoch" (float64 seconds derived from the ISO timestamp), "int" (INT64) or "float" (FLOAT)
DECAY_FIELDS = {"timestamp": "epoch", "chunk_index": "int", "token_count": "int", "entropy": "float", "redundancy": "float",
                "domain_density": "float"}

_LOG2E = float.fromhex("0x1.71547652b82fep+0")
_LN2_HI = float.fromhex("0x1.62e42fee00000p-1")
_LN2_LO = float.fromhex("0x1.a39ef35793c76p-33")
_EXP_SERIES = tuple(1.0 / math.factorial(i) for i in range(14))   # i! <= 13! is exact in a double: each quotient correctly rounded
_EPOCH = datetime(1970, 1, 1, tzinfo=timezone.utc)
_NAN = float("nan")


def canonical_exp(x: float) -> float:
    """The exponential of the decay ranker for x <= 0: no table, no library call, the same bits as csrc/decay.h.
    x = k ln2 + r, a 13th-degree Taylor polynomial in r, an exact scaling by 2^k.  Within 1 ulp of math.exp on
    [-708, 0) (sampled); NaN and x < -708 give 0.0, x >= 0 gives 1.0."""
    x = float(x)
    if x != x:
        return 0.0
    if x >= 0.0:
        return 1.0
    if x < -708.0:
        return 0.0
    k = float(round(x * _LOG2E))          # round(): ties to even, as rint
    r = (x - k * _LN2_HI) - k * _LN2_LO
    p = _EXP_SERIES[13]
    for i in range(12, -1, -1):
        p = _EXP_SERIES[i] + r * p
    return math.ldexp(p, int(k))


def epoch_seconds(text: Any) -> float:
    """ISO-8601 text -> seconds since 1970-01-01 UTC as a float; a naive time is taken as UTC.  NaN for the empty string
    and for anything datetime.fromisoformat refuses ("the row has no value")."""
    if not isinstance(text, str) or not text:
        return _NAN
    try:
        dt = datetime.fromisoformat(text)
    except ValueError:
        return _NAN
    if dt.tzinfo is None:
        dt = dt.replace(tzinfo=timezone.utc)
    return (dt - _EPOCH).total_seconds()


def _number(name: str, value: Any) -> float:
    if isinstance(value, bool) or not isinstance(value, (int, float)):
        raise ValueError(f"{name} must be a number, got {value!r}")
    value = float(value)
    if not math.isfinite(value):
        raise ValueError(f"{name} must be finite, got {value!r}")
    return value


@dataclass(frozen=True)
class DecayRanker:
    """search(..., ranker=DecayRanker(...)) / RetrievalConfig(decay=DecayRanker(...)).

    field          timestamp, chunk_index, token_count, entropy, redundancy or domain_density
    function       "gauss", "exp" or "linear"
    origin         where the factor is 1.0.  timestamp: epoch seconds, a datetime, an ISO string, or None = now (read
                   once per request); the other fields need a number
    scale          the distance (beyond offset) at which the factor has fallen to `decay`; timestamp: seconds
    offset         distances up to offset keep factor 1.0
    decay          the factor at distance offset + scale, in (0, 1)
    normalization  "activation" (by the collection's metric), "minmax" or "none" (the raw score; refused on L2)
    candidates     rerank the best max(top_k, candidates) rows of the plain ranking instead of the best top_k
    """
    field: str
    function: str = "gauss"
    origin: Any = None
    scale: float = None
    offset: float = 0.0
    decay: float = 0.5
    normalization: str = "activation"
    candidates: Optional[int] = None

    def __post_init__(self):
        if not isinstance(self.field, str) or self.field not in DECAY_FIELDS:
            raise ValueError(f"field must be one of {', '.join(DECAY_FIELDS)}, got {self.field!r}")
        if not isinstance(self.function, str) or self.function not in DECAY_FUNCTIONS:
            raise ValueError(f"function must be one of {', '.join(DECAY_FUNCTIONS)}, got {self.function!r}")
        if self.scale is None or _number("scale", self.scale) <= 0.0:
            raise ValueError(f"scale must be a number > 0, got {self.scale!r}")
        if _number("offset", self.offset) < 0.0:
            raise ValueError(f"offset must be >= 0, got {self.offset!r}")
        if not 0.0 < _number("decay", self.decay) < 1.0:
            raise ValueError(f"decay must lie inside (0, 1), got {self.decay!r}")
        if self.normalization not in DECAY_NORMALIZATIONS:
            raise ValueError(f"normalization must be one of {', '.join(DECAY_NORMALIZATIONS)}, got {self.normalization!r}")
        if self.candidates is not None and (isinstance(self.candidates, bool) or not isinstance(self.candidates, int)
                                            or self.candidates < 1):
            raise ValueError(f"candidates must be an integer >= 1 or None, got {self.candidates!r}")
        if self.origin is None:
            if self.field != "timestamp":
                raise ValueError(f"origin=None means now and is valid only for field='timestamp', not {self.field!r}")
        elif self.field == "timestamp" and isinstance(self.origin, (str, datetime)):
            if not math.isfinite(self._origin_value()):
                raise ValueError(f"origin is not an ISO-8601 time: {self.origin!r}")
        else:
            _number("origin", self.origin)

    def _origin_value(self) -> float:
        if self.origin is None:
            return time.time()
        if isinstance(self.origin, datetime):
            dt = self.origin if self.origin.tzinfo is not None else self.origin.replace(tzinfo=timezone.utc)
            return (dt - _EPOCH).total_seconds()
        if isinstance(self.origin, str):
            return epoch_seconds(self.origin)
        return float(self.origin)

    def operands(self) -> Tuple[float, float, float, int]:
        """(origin, offset, coef, func): what travels to the device for one request.  coef is computed here, with
        math.log on Python floats, so that the device needs no logarithm."""
        scale, decay = float(self.scale), float(self.decay)
        if self.function == "gauss":
            coef = math.log(decay) / (scale * scale)
        elif self.function == "exp":
            coef = math.log(decay) / scale
        else:
            coef = (1.0 - decay) / scale
        return (self._origin_value(), float(self.offset), coef, DECAY_FUNCTIONS[self.function])

    def window(self, top_k: int) -> int:
        """W: how deep the plain ranking is read before the rerank."""
        return max(int(top_k), int(self.candidates or top_k))

    def norm_code(self, metric: str, fused: bool = False) -> int:
        """HR_NORM_* (or HR_NORM_NONE) for a list ranked by `metric`.  fused = the list holds RRF / weighted fused scores,
        which are not renormalised: "activation" means identity there."""
        if self.normalization == "minmax":
            return HR_NORM_MINMAX_DIST if not fused and str(metric).upper() == "L2" else HR_NORM_MINMAX
        if fused or self.normalization == "none":
            if not fused and str(metric).upper() == "L2":
                raise ValueError("normalization='none' is refused on an L2 collection, where a smaller score is the better one")
            return HR_NORM_NONE
        from .retrieval import norm_code
        return norm_code(metric, "activation")


def decay_factor(operands: Sequence[float], v: float) -> float:
    """The decay factor of field value v for (origin, offset, coef, func): the table of include/hbmrag.h."""
    origin, offset, coef, func = operands
    v = float(v)
    if v != v:
        return 0.0
    a = abs(v - origin)
    u = a - offset
    d = u if u > 0.0 else 0.0
    if func == HR_DECAY_GAUSS:
        return canonical_exp(coef * (d * d))
    if func == HR_DECAY_EXP:
        return canonical_exp(coef * d)
    if func == HR_DECAY_LINEAR:
        g = 1.0 - d * coef
        return g if g > 0.0 else 0.0
    return 0.0


def normalise(scores: Sequence[float], code: int) -> List[float]:
    """retrieval.normalise_scores for scores that are already doubles (fp32 scores widened, or fp64 fused scores), plus
    the identity HR_NORM_NONE."""
    if code == HR_NORM_NONE:
        return [float(x) for x in scores]
    from .retrieval import normalise_scores
    return normalise_scores(scores, code, widened=True)


def decay_rerank(ids: Sequence[int], scores: Sequence[float], values: Sequence[float], operands: Sequence[float], norm: int,
                 k_out: int) -> Tuple[List[int], List[int], List[float]]:
    """Host restatement of hr_decay_rerank_dev for ONE list: ids / scores = the list's valid prefix, values[i] = the
    field value of ids[i] as a float (NaN where the row has none or lies outside the column).
    -> (positions, ids, final scores) of the first k_out entries in the stable descending order of final; shorter than
    k_out when the list is (the device pads with -1 / -1 / 0.0)."""
    n = len(ids)
    ns = normalise(scores, norm)
    final = [ns[i] * decay_factor(operands, values[i]) for i in range(n)]
    order = sorted(range(n), key=lambda i: final[i], reverse=True)[:k_out]   # stable: ties keep input order
    return order, [ids[i] for i in order], [final[i] for i in order]
