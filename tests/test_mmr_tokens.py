"""MMR on the device, the host side (no GPU): the token-set column the kernel reads, and who is asked for the
one-round MMR path.

The reference diversifies on `set(content.lower().split())` (retrieval.py:495); columns.TokenSetColumn keeps exactly
those sets as sorted int32 ids of a collection-wide dictionary."""
import asyncio

import numpy as np
import pytest

from advanced_rag import HybridRetriever, MilvusIndexManager, RetrievalConfig
from advanced_rag.columns import PayloadColumns, TokenSetColumn

CONTENTS = [
    "İstanbul Straße",                       # lower() maps U+0130 to two code points; ß stays
    "istanbul STRASSE strasse",              # neither equals a token of the row above
    "tab\tseparated\twords tab",
    "line one\nline two\r\nline three",
    "em\u2003space\u2003\u2003between words",        # U+2003 is whitespace to str.split
    "",
    "   \t\n ",
    "repeat repeat REPEAT Repeat rePeat",
    "ǅ Ǆ ǆ ǅ",                               # three cases of one letter: one token after lower()
    "nbsp\u00a0joined x\u200bzero-width",             # U+00A0 splits, U+200B does not
    "row 7 topic2 alpha1 common",
]
LATER = ["row 8 topic3 alpha2 common", "İstanbul again", "", "brand new tokens straße"]


def _sets(col):
    back = {i: t for t, i in col.ids.items()}
    assert len(back) == len(col.ids)             # ids are distinct
    return [set(back[int(i)] for i in col.row(r)) for r in range(len(col))]


def test_token_sets_are_the_references_sets():
    col = TokenSetColumn()
    col.extend(CONTENTS)
    assert len(col) == len(CONTENTS)
    assert _sets(col) == [set(c.lower().split()) for c in CONTENTS]
    indptr, tok = col.indptr(), col.tokens()
    assert indptr.dtype == np.int64 and tok.dtype == np.int32 and indptr.shape == (len(CONTENTS) + 1,)
    assert indptr[0] == 0 and indptr[-1] == tok.shape[0]
    for r in range(len(col)):
        row = tok[indptr[r]: indptr[r + 1]]
        assert row.tolist() == col.row(r).tolist()
        assert (np.diff(row) > 0).all()                                  # ascending and unique
        assert len(row) == len(set(CONTENTS[r].lower().split()))
    assert col.row(5).size == 0 and col.row(6).size == 0
    # first-seen order: ids are dense, and no row uses an id before the rows above (and itself) introduced it
    assert sorted(col.ids.values()) == list(range(len(col.ids)))
    seen = 0
    for r in range(len(col)):
        new = [int(i) for i in col.row(r) if i >= seen]
        assert new == list(range(seen, seen + len(new)))
        seen += len(new)


def test_extend_leaves_earlier_rows_and_ids_untouched():
    cols = PayloadColumns()
    cols["content"].extend(CONTENTS)
    col = cols.token_sets()
    before_rows = [col.row(r).tolist() for r in range(len(col))]
    before_ids = dict(col.ids)
    cols["content"].extend(LATER)
    assert len(col) == len(CONTENTS)                  # lazily: nothing happens until the next use
    again = cols.token_sets()
    assert again is col and len(col) == len(CONTENTS) + len(LATER)
    assert [col.row(r).tolist() for r in range(len(CONTENTS))] == before_rows
    assert {t: col.ids[t] for t in before_ids} == before_ids
    assert min(i for t, i in col.ids.items() if t not in before_ids) == len(before_ids)
    assert _sets(col) == [set(c.lower().split()) for c in CONTENTS + LATER]
    # the same contents in one go give the same column: tokenising in pieces changes nothing
    whole = TokenSetColumn()
    whole.extend(CONTENTS + LATER)
    assert whole.ids == col.ids and whole.tokens().tolist() == col.tokens().tolist()
    assert whole.indptr().tolist() == col.indptr().tolist()
    assert cols.token_sets() is col and len(col) == len(CONTENTS) + len(LATER)     # nothing new: nothing redone
    assert "token_sets" not in list(cols) and all(k != "token_sets" for k, _ in cols.items())   # not a payload field


def test_too_many_distinct_tokens_are_refused(monkeypatch):
    monkeypatch.setattr(TokenSetColumn, "MAX_TOKENS", 3)
    col = TokenSetColumn()
    col.extend(["a b", "c a"])
    with pytest.raises(ValueError, match="distinct tokens"):
        col.extend(["d"])
    assert TokenSetColumn.__dict__["MAX_TOKENS"] == 3 and len(col.ids) == 3


class _OneRoundStandIn:
    """An index manager with the one-round entry point but WITHOUT `mmr_on_device` (a duck-typed manager written before
    the option existed): it must never be asked for an MMR request."""

    def __init__(self):
        self.collections = {"semantic_index": 1, "sparse_index": 1}
        self.hybrid_calls, self.search_calls = [], 0

    async def _generate_semantic_embedding(self, text):
        return np.ones(4, np.float32)

    async def _generate_sparse_embedding(self, text):
        return {"indices": [1], "values": [1.0]}

    async def hybrid_search(self, dense, sparse, top_k, filters, weights, rrf_k=60, semantic_params=None, sparse_params=None):
        self.hybrid_calls.append(top_k)
        return self._fused()

    @staticmethod
    def _fused():
        return [({"id": f"h{i}", "content": f"c{i}", "score": 1.0 - 0.1 * i, "metadata": {}}, 0.5 - 0.01 * i, 3)
                for i in range(3)]

    async def search(self, query_embedding, collection_name, top_k=20, filters=None, search_params=None):
        self.search_calls += 1
        return [{"id": f"g{i}", "content": f"shared w{i}", "score": 1.0 - 0.1 * i, "metadata": {}} for i in range(4)]


def test_retriever_keeps_declining_mmr_for_a_manager_without_the_option():
    mgr = _OneRoundStandIn()
    retr = HybridRetriever(mgr, RetrievalConfig(top_k=20))
    out = asyncio.run(retr.retrieve("plain statement", profile_hint="troubleshooting"))
    assert retr.config.enable_mmr and mgr.hybrid_calls == [] and mgr.search_calls == 2
    assert [o["id"] for o in out][:1] == ["g0"] and len(out) == 4
    assert asyncio.run(retr._retrieve_one_round("q", np.ones(4, np.float32), {"indices": [1], "values": [1.0]}, None)) is None
    # a profile without MMR still takes the one-round path of the same manager (whose entry point knows no mmr_lambda)
    out = asyncio.run(retr.retrieve("plain statement", profile_hint="summary"))
    assert mgr.hybrid_calls == [40] and mgr.search_calls == 2 and [o["id"] for o in out] == ["h0", "h1", "h2"]


def test_retriever_asks_a_manager_that_offers_mmr_on_device():
    class Offers(_OneRoundStandIn):
        mmr_on_device = True

        async def hybrid_search(self, dense, sparse, top_k, filters, weights, rrf_k=60, semantic_params=None,
                                sparse_params=None, mmr_lambda=None):
            self.hybrid_calls.append((top_k, mmr_lambda))
            return None if mmr_lambda == 0.8 else self._fused()

    mgr = Offers()
    retr = HybridRetriever(mgr, RetrievalConfig(top_k=20))
    out = asyncio.run(retr.retrieve("plain statement", profile_hint="troubleshooting"))
    assert mgr.hybrid_calls[0] == (30, 0.5) and mgr.search_calls == 0 and [o["id"] for o in out] == ["h0", "h1", "h2"]
    out = asyncio.run(retr.retrieve("plain statement", profile_hint="analysis"))     # declined: the general path answers
    assert mgr.hybrid_calls[1] == (30, 0.8) and mgr.search_calls == 2 and out[0]["id"] == "g0"
    asyncio.run(retr.retrieve("plain statement", profile_hint="summary"))
    assert mgr.hybrid_calls[2] == (40, None)


def test_hybrid_search_declines_mmr_unless_the_manager_was_created_for_it():
    mgr = MilvusIndexManager(connect=False)
    assert mgr.mmr_on_device is False
    mgr._coalescer = lambda coll: pytest.fail("a declined request must not reach the front")
    args = (np.ones(4, np.float32), {"indices": [1], "values": [1.0]})
    assert asyncio.run(mgr.hybrid_search(*args, top_k=30, filters=None, weights=(0.7, 0.3), mmr_lambda=0.5)) is None
    assert MilvusIndexManager(connect=False, mmr_on_device=True).mmr_on_device is True
    with pytest.raises(TypeError):
        MilvusIndexManager("localhost", 19530, True, 4, 1536, 10000, 768, False, True)     # no ninth positional: keyword-only
