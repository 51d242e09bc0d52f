"""Expected row masks of filter expressions beyond the flat conjunction, composed from the oracle (a helper, not a test).

`oracle.filter_mask` evaluates one conjunctive expression.  A test states what an expression means as a small tree written
by hand beside the expression text -- C("field OP literal"), IN("field", literal, ...), AND / OR / NOT -- and `expected`
evaluates it: a comparison through the oracle, a membership leaf as the `|` of the oracle's `==` masks of its members (the
literals are given as they stand in an expression, quotes and escapes included), the rest with numpy's & | ~.  Nothing here
reads advanced_rag.filters."""
import numpy as np

import oracle


def C(term):
    return ("cmp", term)


def IN(field, *literals):
    return ("in", field, literals)


def AND(*xs):
    return ("and",) + xs


def OR(*xs):
    return ("or",) + xs


def NOT(x):
    return ("not", x)


def expected(spec, columns, n):
    kind = spec[0]
    if kind == "cmp":
        return oracle.filter_mask(spec[1], columns, n)
    if kind == "in":
        keep = np.zeros(n, dtype=bool)
        for lit in spec[2]:
            keep |= oracle.filter_mask(f"{spec[1]} == {lit}", columns, n)
        return keep
    if kind == "not":
        return ~expected(spec[1], columns, n)
    parts = [expected(x, columns, n) for x in spec[1:]]
    out = parts[0].copy()
    for p in parts[1:]:
        out = (out & p) if kind == "and" else (out | p)
    return out
