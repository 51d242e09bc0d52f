"""Filter expressions -> row bitmask.

HybridRetriever._build_filter_expression (reference retrieval.py:573-632) emits
Milvus boolean expressions of the form
    field OP value and field OP value ...
with OP in {>=, <=, >, <, ==, !=}, values int/float/bool literals or
double-quoted strings with \\ and \" escapes, over the scalar fields of the
collection schema (indexing.py:191-225).  Milvus evaluates them server-side;
here they become a per-row predicate over host-side columns and are handed to
the kernels as a packed bitmask (bit r%8 of byte r/8).

A pymilvus caller writes more than conjunctions, so `parse_tree` also takes
    field in [literal, ...]   field not in [...]   or / ||   not / !   ( ... )
with Milvus' precedence (not > and > or).  `parse` keeps to the flat
conjunction; `evaluate` and `fields` take either form.  `parse_tree` also takes the
keyword filter of Milvus 2.5,
    TEXT_MATCH(content, "words"[, minimum_should_match=m])
over the words of `content` (`analyze`, the BM25 tokenizer): a row passes iff at least
m (default 1) distinct words of the query are among its words.  The rest of Milvus'
language (like, PHRASE_MATCH, arithmetic, a < f < b, field-to-field comparisons,
JSON and array functions) is refused.
"""
from __future__ import annotations

import re
from typing import Any, Dict, List, Optional, Tuple

import numpy as np

_OPS = (">=", "<=", "==", "!=", ">", "<")
NUMERIC_FIELDS = {"chunk_index": np.int64, "token_count": np.int64, "entropy": np.float32,
                  "redundancy": np.float32, "domain_density": np.float32}
STRING_FIELDS = ("id", "chunk_id", "doc_id", "timestamp")
TEXT_FIELDS = ("content",)             # what TEXT_MATCH analyses
MATCH_MAX = 16384                      # minimum_should_match, and the word ids one expression can carry to the device
_ANALYZER = re.compile(r"\w+")


def analyze(text: str) -> List[str]:
    """The words of a text as TEXT_MATCH sees them, in order: maximal runs of Unicode word characters of the lower-cased
    text — what the BM25 modality tokenises with (bm25._WORD), so "Timeout," and "timeout" are one word."""
    return _ANALYZER.findall(text.lower())


def match_rows(contents, text: str, m: int) -> np.ndarray:
    """TEXT_MATCH over a sequence of str: row r passes iff at least m distinct words of `text` are among its words."""
    words = set(analyze(text))
    if not words or m > len(words):
        return np.zeros(len(contents), dtype=bool)
    return np.fromiter((len(words.intersection(analyze(c))) >= m for c in contents), dtype=bool, count=len(contents))


def _split_terms(expr: str) -> List[str]:
    """Split on ' and ' that is not inside a double-quoted string."""
    terms, buf, in_str, i = [], [], False, 0
    while i < len(expr):
        ch = expr[i]
        if in_str:
            buf.append(ch)
            if ch == "\\" and i + 1 < len(expr):
                buf.append(expr[i + 1])
                i += 1
            elif ch == '"':
                in_str = False
        elif ch == '"':
            in_str = True
            buf.append(ch)
        elif expr.startswith(" and ", i):
            terms.append("".join(buf))
            buf = []
            i += 4
        else:
            buf.append(ch)
        i += 1
    if in_str:
        raise ValueError(f"unterminated string in filter expression: {expr!r}")
    terms.append("".join(buf))
    return [t.strip() for t in terms if t.strip()]


def _unquote(tok: str) -> str:
    out, i = [], 1
    while i < len(tok) - 1:
        if tok[i] == "\\" and i + 1 < len(tok) - 1:
            out.append(tok[i + 1])
            i += 2
        else:
            out.append(tok[i])
            i += 1
    return "".join(out)


def _string_end(text: str, i: int) -> int:
    """Index just behind the double-quoted string that starts at text[i], or -1 when it does not end."""
    i += 1
    while i < len(text):
        if text[i] == "\\" and i + 1 < len(text):
            i += 2
        elif text[i] == '"':
            return i + 1
        else:
            i += 1
    return -1


_TERM = re.compile(r"^\s*([A-Za-z_]\w*)\s*(>=|<=|==|!=|>|<)\s*(.+?)\s*$", re.S)


def parse(expr: str) -> List[Tuple[str, str, Any]]:
    """-> [(field, op, python value)].  The operator is the one right after the field name: a quoted value
    may itself contain ' >= ', ' and ' or escaped quotes (doc_id == "a >= b")."""
    parsed = []
    for term in _split_terms(expr):
        m = _TERM.match(term)
        if m is None:
            raise ValueError(f"cannot parse filter term: {term!r}")
        field, op, raw = m.group(1), m.group(2), m.group(3)
        if raw.startswith('"') and raw.endswith('"') and len(raw) >= 2:
            if _string_end(raw, 0) != len(raw):   # `"a" or doc_id == "b"` is no literal (it used to be read as one string)
                raise ValueError(f"bad literal in filter term: {term!r}")
            value: Any = _unquote(raw)
        elif raw in ("True", "true"):
            value = True
        elif raw in ("False", "false"):
            value = False
        else:
            try:
                value = int(raw)
            except ValueError:
                try:
                    value = float(raw)
                except ValueError:
                    raise ValueError(f"bad literal in filter term: {term!r}")
        parsed.append((field, op, value))
    return parsed


INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1


def numeric_literal(field: str, op: str, value: Any, kind: str):
    """The literal of `field op value` as the column compares it, or ValueError naming the term when the literal does not
    fit (Milvus refuses such an expression; wrapping it into the field would answer another one).
    kind "i" (INT64 field): an integer literal stays an int and must lie in [-2^63, 2^63 - 1]; a float literal stays a float
    (the column is compared as float64, which holds every float literal).
    kind "f" (FLOAT field): the literal rounded to float32; one beyond float32's range becomes +-inf, as numpy rounds it
    (`entropy < 1e39` keeps every finite row), but an integer too large for a float at all is refused."""
    if kind == "i":
        if isinstance(value, float):
            return value
        if not INT64_MIN <= int(value) <= INT64_MAX:
            raise ValueError(f"integer literal out of the int64 range in filter term: {field} {op} {value}")
        return int(value)
    try:
        as_float = float(value)
    except OverflowError:
        raise ValueError(f"literal out of the floating-point range in filter term: {field} {op} {value}") from None
    with np.errstate(over="ignore"):
        return np.float32(as_float)


def _compare(col: np.ndarray, op: str, value: Any) -> np.ndarray:
    if op == "==":
        return col == value
    if op == "!=":
        return col != value
    if op == ">=":
        return col >= value
    if op == "<=":
        return col <= value
    if op == ">":
        return col > value
    return col < value


def _leaf_mask(node, columns: Dict[str, np.ndarray]) -> np.ndarray:
    """Row predicate of one leaf: ("cmp", field, op, value), ("in", field, values) or ("match", field, text, m) — the last
    over columns["content"], any sequence of str."""
    field = node[1]
    if field not in columns:
        raise ValueError(f"unknown filter field: {field}")
    col = columns[field]
    if node[0] == "match":
        return match_rows(col, node[2], node[3])
    if node[0] == "in":
        members = list_members(field, node[2], "s" if col.dtype.kind in "US" else "i" if col.dtype.kind in "iu" else "f")
        if not members:
            return np.zeros(col.shape[0], dtype=bool)
        if col.dtype.kind == "f" and col.dtype != np.float32:
            members = [float(v) for v in node[2]]
        return np.isin(col, np.asarray(members, dtype=col.dtype if col.dtype.kind not in "US" else None))
    op, value = node[2], node[3]
    if col.dtype.kind in "US":
        if not isinstance(value, str):
            raise ValueError(f"field {field} is a string column; got {value!r}")
    elif isinstance(value, str):
        raise ValueError(f"field {field} is numeric; got string {value!r}")
    elif col.dtype.kind in "iu":
        value = numeric_literal(field, op, value, "i")
    elif col.dtype.kind == "f":
        rounded = numeric_literal(field, op, value, "f")
        value = rounded if col.dtype == np.float32 else float(value)
    return _compare(col, op, value)


def evaluate_tree(tree, leaf) -> np.ndarray:
    """The tree of parse_tree over boolean arrays: `leaf(node)` gives a leaf's rows, and / or / not are & / | / ~."""
    kind = tree[0]
    if kind == "and":
        return evaluate_tree(tree[1], leaf) & evaluate_tree(tree[2], leaf)
    if kind == "or":
        return evaluate_tree(tree[1], leaf) | evaluate_tree(tree[2], leaf)
    if kind == "not":
        return ~evaluate_tree(tree[1], leaf)
    return leaf(tree)


def evaluate(expr: str, columns: Dict[str, np.ndarray], n_rows: int) -> np.ndarray:
    """Boolean row predicate (length n_rows) of an expression: a conjunction term by term, any other tree with numpy."""
    terms, tree = lower(expr)
    if tree is not None:
        return evaluate_tree(tree, lambda node: _leaf_mask(node, columns))
    keep = np.ones(n_rows, dtype=bool)
    for field, op, value in terms:
        keep &= _leaf_mask(("cmp", field, op, value), columns)
    return keep


# ---------------------------------------------------------------------------------------------------------------------
# the full grammar
#   expr  := or
#   or    := and ( ("or" | "OR" | "||") and )*
#   and   := unary ( ("and" | "AND" | "&&") unary )*
#   unary := ("not" | "NOT" | "!") unary | "(" expr ")" | leaf
#   leaf  := field CMP literal | field ["not"] "in" "[" [ literal ("," literal)* ] "]"
#          | ("TEXT_MATCH" | "text_match") "(" field "," string [ "," "minimum_should_match" "=" integer ] ")"
# Trees: ("cmp", field, op, value) | ("in", field, [values]) | ("match", field, text, m) | ("not", t) | ("and", a, b) |
# ("or", a, b), and / or left-associative; `field not in [..]` is ("not", ("in", ..)); m = 1 without the option.

_KEYWORDS = {"and": "and", "AND": "and", "&&": "and", "or": "or", "OR": "or", "||": "or", "not": "not", "NOT": "not",
             "!": "not", "in": "in", "IN": "in"}
_IDENT = re.compile(r"[A-Za-z_]\w*$")
_WORD = re.compile(r"[\w.+\-]+")       # identifiers, keywords and numeric literals (1e-3, -inf, 1_000)
_PUNCT = ("&&", "||", ">=", "<=", "==", "!=", ">", "<", "!", "(", ")", "[", "]", ",", "=")   # "=": only inside TEXT_MATCH(...)
_MATCH_NAMES = ("TEXT_MATCH", "text_match")


def _tokens(expr: str) -> List[Tuple[str, str, int, int]]:
    """-> [(kind, text, start, end)], kind one of "str" (text = the quoted source), "word", "cmp", or the keyword /
    punctuation itself.  What stands inside a quoted string is part of the string."""
    out, i = [], 0
    while i < len(expr):
        ch = expr[i]
        if ch.isspace():
            i += 1
        elif ch == '"':
            end = _string_end(expr, i)
            if end < 0:
                raise ValueError(f"unterminated string in filter expression: {expr!r}")
            out.append(("str", expr[i:end], i, end))
            i = end
        else:
            m = _WORD.match(expr, i)
            if m is not None:
                text = m.group(0)
                out.append((_KEYWORDS.get(text, "word"), text, i, m.end()))
                i = m.end()
                continue
            for p in _PUNCT:
                if expr.startswith(p, i):
                    out.append(("cmp" if p in _OPS else _KEYWORDS.get(p, p), p, i, i + len(p)))
                    i += len(p)
                    break
            else:
                raise ValueError(f"cannot parse filter expression at {expr[i:i + 12]!r}: {expr!r}")
    return out


def _literal(tok, term: str) -> Any:
    kind, text = tok[0], tok[1]
    if kind == "str":
        return _unquote(text)
    if kind == "word":
        if text in ("True", "true"):
            return True
        if text in ("False", "false"):
            return False
        try:
            return int(text)
        except ValueError:
            try:
                return float(text)
            except ValueError:
                pass
    raise ValueError(f"bad literal in filter term: {term!r}")


def list_members(field: str, values: List[Any], kind: str) -> List[Any]:
    """The members of `field in [values]` as a column of `kind` ("s" string, "i" INT64, "f" FLOAT) compares them, or
    ValueError naming the term: strings for a string field; integers within int64 for an INT64 field (a float literal is
    refused: no row equals 2.5, and Milvus refuses the list); numbers rounded to float32 for a FLOAT field."""
    term = f"{field} in {_show_list(values)}"
    strings = [isinstance(v, str) for v in values]
    if any(strings) and not all(strings):
        raise ValueError(f"list mixes strings and numbers in filter term: {term}")
    if kind == "s":
        if values and not all(strings):
            raise ValueError(f"field {field} is a string column; got a number in filter term: {term}")
        return list(values)
    if any(strings):
        raise ValueError(f"field {field} is numeric; got a string in filter term: {term}")
    if kind == "i":
        if any(isinstance(v, float) for v in values):
            raise ValueError(f"field {field} is an INT64 field; got a float literal in filter term: {term}")
        return [numeric_literal(field, "in", v, "i") for v in values]
    return [numeric_literal(field, "in", v, "f") for v in values]


def _show_list(values) -> str:
    return "[" + ", ".join('"' + v.replace("\\", "\\\\").replace('"', '\\"') + '"' if isinstance(v, str) else str(v)
                           for v in values) + "]"


class _Parser:
    def __init__(self, expr: str):
        self.expr, self.toks, self.i = expr, _tokens(expr), 0

    def peek(self) -> str:
        return self.toks[self.i][0] if self.i < len(self.toks) else "end"

    def text_from(self, first: int, last: Optional[int] = None) -> str:
        """The source from token `first` up to and including token `last` (default: the one just read)."""
        last = min(self.i - 1 if last is None else last, len(self.toks) - 1)
        return self.expr[self.toks[first][2]: self.toks[last][3]] if first <= last else self.expr

    def parse(self):
        if not self.toks:
            raise ValueError(f"empty filter expression: {self.expr!r}")
        tree = self.or_()
        if self.peek() == ")":
            raise ValueError(f"unbalanced parentheses in filter expression: {self.expr!r}")
        if self.peek() != "end":
            raise ValueError(f"cannot parse filter term: {self.text_from(self.start, len(self.toks) - 1)!r}")
        return tree

    def or_(self):
        tree = self.and_()
        while self.peek() == "or":
            self.i += 1
            tree = ("or", tree, self.and_())
        return tree

    def and_(self):
        tree = self.unary()
        while self.peek() == "and":
            self.i += 1
            tree = ("and", tree, self.unary())
        return tree

    def unary(self):
        kind = self.peek()
        if kind == "not":
            self.i += 1
            return ("not", self.unary())
        if kind == "(":
            self.i += 1
            tree = self.or_()
            if self.peek() != ")":
                raise ValueError(f"unbalanced parentheses in filter expression: {self.expr!r}")
            self.i += 1
            return tree
        return self.leaf()

    def leaf(self):
        self.start = start = self.i
        if self.peek() == "end":
            raise ValueError(f"filter expression ends where a term is expected: {self.expr!r}")
        tok = self.toks[self.i]
        self.i += 1
        if tok[0] != "word" or not _IDENT.match(tok[1]) or tok[1] in ("True", "true", "False", "false"):
            raise ValueError(f"cannot parse filter term: {self.text_from(start, min(start + 2, len(self.toks) - 1))!r}")
        field, kind = tok[1], self.peek()
        if field in _MATCH_NAMES and kind == "(":
            return self.match(start)
        if kind == "cmp":
            op = self.toks[self.i][1]
            self.i += 1
            if self.peek() == "end":
                raise ValueError(f"bad literal in filter term: {self.text_from(start)!r}")
            self.i += 1
            return ("cmp", field, op, _literal(self.toks[self.i - 1], self.text_from(start)))
        negate = kind == "not"
        if negate:
            self.i += 1
        if self.peek() != "in":
            raise ValueError(f"cannot parse filter term: {self.text_from(start, min(self.i, len(self.toks) - 1))!r} "
                             "(expected a comparison or [not] in [...])")
        self.i += 1
        if self.peek() != "[":
            raise ValueError(f"cannot parse filter term: {self.text_from(start, min(self.i, len(self.toks) - 1))!r} "
                             "(expected a [list] after in)")
        self.i += 1
        close = next((j for j in range(self.i, len(self.toks)) if self.toks[j][0] == "]"), len(self.toks) - 1)
        term = self.text_from(start, close)
        values: List[Any] = []
        if self.peek() == "]":
            self.i += 1
        else:
            while True:
                if self.peek() == "]" and values:
                    raise ValueError(f"trailing comma in filter term: {term!r}")
                if self.peek() not in ("str", "word"):
                    raise ValueError(f"bad list in filter term: {term!r}")
                self.i += 1
                values.append(_literal(self.toks[self.i - 1], term))
                sep = self.peek()
                self.i += 1
                if sep == "]":
                    break
                if sep != ",":
                    raise ValueError(f"bad list in filter term: {term!r}")
        # what the field's type refuses is refused here, before any evaluator sees the tree
        if field in NUMERIC_FIELDS or field in STRING_FIELDS:
            list_members(field, values, "s" if field in STRING_FIELDS else "i" if NUMERIC_FIELDS[field] is np.int64 else "f")
        else:
            list_members(field, values, "s" if values and isinstance(values[0], str) else "f")
        node = ("in", field, values)
        return ("not", node) if negate else node


    def match(self, start: int):
        """TEXT_MATCH ( field , "text" [, minimum_should_match = integer] ) with the name already read."""
        close = next((j for j in range(self.i, len(self.toks)) if self.toks[j][0] == ")"), len(self.toks) - 1)
        term = self.text_from(start, close)

        def take(kind: str, what: str):
            if self.peek() != kind:
                raise ValueError(f"{what} in filter term: {term!r}")
            self.i += 1
            return self.toks[self.i - 1]

        take("(", "expected (")
        field = take("word", "expected a field name after TEXT_MATCH(")[1]
        if not _IDENT.match(field):
            raise ValueError(f"expected a field name after TEXT_MATCH( in filter term: {term!r}")
        if field not in TEXT_FIELDS:
            raise ValueError(f"TEXT_MATCH analyses only the field content, not {field}, in filter term: {term!r}")
        if self.peek() != ",":
            raise ValueError(f"TEXT_MATCH needs a field and a quoted text; the text is missing in filter term: {term!r}")
        self.i += 1
        if self.peek() in (")", "end"):
            raise ValueError(f"TEXT_MATCH needs a field and a quoted text; the text is missing in filter term: {term!r}")
        text = _unquote(take("str", "the text of TEXT_MATCH must be a double-quoted string")[1])
        m = 1
        if self.peek() == ",":
            self.i += 1
            option = take("word", "expected minimum_should_match=<integer> after the text")[1]
            if option != "minimum_should_match":
                raise ValueError(f"unknown TEXT_MATCH option {option!r} (only minimum_should_match) in filter term: {term!r}")
            take("=", "expected = after minimum_should_match")
            raw = take("word", "minimum_should_match needs an integer")[1]
            if not re.fullmatch(r"[0-9]+", raw) or not 1 <= int(raw) <= MATCH_MAX:
                raise ValueError(f"minimum_should_match must be an integer from 1 to {MATCH_MAX}, got {raw} in filter term: {term!r}")
            m = int(raw)
        if self.peek() != ")":
            raise ValueError(f"missing ) in filter term: {term!r}")
        self.i += 1
        return ("match", field, text, m)


def parse_tree(expr: str):
    """The expression as a tree (see the grammar above), or ValueError naming the offending term."""
    return _Parser(expr).parse()


def conjunction_terms(tree) -> Optional[List[Tuple[str, str, Any]]]:
    """[(field, op, value)] when the tree is a flat conjunction of comparisons (what `parse` returns), else None."""
    if tree[0] == "cmp":
        return [tree[1:]]
    if tree[0] == "and":
        left, right = conjunction_terms(tree[1]), conjunction_terms(tree[2])
        if left is not None and right is not None:
            return left + right
    return None


def lower(expr: str):
    """-> (terms, None) for a flat conjunction of comparisons (however it is spelled: `and`, `AND`, `&&`, parentheses),
    (None, tree) for every other expression."""
    try:
        return parse(expr), None
    except ValueError:
        pass
    tree = parse_tree(expr)
    terms = conjunction_terms(tree)
    return (terms, None) if terms is not None else (None, tree)


def leaves(tree) -> List[tuple]:
    if tree[0] in ("cmp", "in", "match"):
        return [tree]
    return [leaf for child in tree[1:] for leaf in leaves(child)]


def fields(expr: str) -> set:
    """The field names an expression of either form mentions."""
    terms, tree = lower(expr)
    return {t[0] for t in terms} if tree is None else {leaf[1] for leaf in leaves(tree)}


def pack(keep: np.ndarray) -> np.ndarray:
    return np.packbits(keep.astype(np.uint8), bitorder="little")
