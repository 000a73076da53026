"""CPU: ragmeup_amd/records.py, the one record table behind the dense store and the BM25 retriever -- the same conditions over the same
records give both owners the rows of a brute-force walk; the seqlock's read and write side, without timing; the grouping of one condition
per query against the loops it replaced; and the module graph (bm25 does not need vectorstore)."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from ragmeup_amd.records import Seqlock, consistent, flatten_groups, group_conditions
from tests.test_bm25_groups_cpu import _Index
from tests.test_subset_cpu import HashEmbeddings, NumpyStore

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- one table, both owners ------------------------------------------------------------------------------------------------------------
METAS = [
    {"source": "a.pdf", "page": 0, "score": 0.5},
    {"source": "b.pdf", "page": 1, "score": 1.5, "tags": ["x", "y"]},          # a list as value: unhashable
    {"source": "a.pdf", "page": 2, "tags": "x"},
    {"page": 3, "score": 2},                                                     # no `source`: it holds None
    {"source": None, "page": 4},                                                 # ... and an explicit None
    {"source": "c.pdf", "page": 0, "tags": ["x", "y"]},
    {"source": "c.pdf", "page": 1, "tags": {"k": "v"}},                          # a dict as value
    {"source": "a.pdf", "page": 2, "score": 2.0, "tags": "x"},
    {"source": "b.pdf", "page": 3, "tags": ["y"]},
    {"source": "b.pdf", "page": 4, "score": 0.5, "tags": "y"},
    {"source": "d.pdf", "page": 0},
    {"source": "a.pdf", "page": 1, "tags": ["x", "y"]},
    {"source": "c.pdf", "page": 2, "score": 1.5},
    {"source": "a.pdf", "page": 3, "tags": {"k": "v"}},
    {"source": "b.pdf", "page": 4},
    {"source": "a.pdf", "page": 0, "score": 2},
]
PKS = ["id-%d" % i for i in range(len(METAS))]
TEXTS = ["record %d" % i for i in range(len(METAS))]
DEAD = [2, 5, 14]
CONDS = [
    [("source", ["a.pdf"])],                                                     # one value
    [("source", ["a.pdf", "c.pdf", "zzz"])],                                     # several values
    [("source", ["a.pdf", "b.pdf"]), ("page", [1, 3])],                          # two fields
    [("source", ["nowhere.pdf"])],                                               # a value nobody holds
    [("source", [None])],                                                        # missing and None alike
    [("tags", ["x"])],                                                           # hashable holders only: "x" is no element of a held list
    [("tags", [["x", "y"]])],                                                    # a list-valued field matched by element ...
    [("tags", ["x", "y"])],                                                      # ... and by the whole list (and the plain "x" / "y")
    [("tags", [{"k": "v"}, "y"])],
    [("score", [2])], [("score", [0.5, 1.5])],                                   # ints and floats: 2 == 2.0
    [("pk", ["id-3", "id-5", "id-15", "id-99"])],                                # the primary key (id-5 is dead)
    [("pk", ["id-7"]), ("source", ["a.pdf"])],
    [("tags", [["x", "y"]]), ("source", ["a.pdf", "b.pdf"])],
    [],                                                                          # no conditions: all live rows
]


def brute(conds):
    out = []
    for r, (pk, meta) in enumerate(zip(PKS, METAS)):
        ok = r not in DEAD
        for field, vals in conds:
            v = pk if field == "pk" else meta.get(field)
            ok = ok and (any(v == x for x in vals) or v == vals)
        if ok:
            out.append(r)
    return out


@pytest.fixture(scope="module")
def owners():
    from ragmeup_amd.bm25 import MI355XBM25Retriever
    store = NumpyStore(embeddings=HashEmbeddings(), collection_name="records-cpu", auto_persist=False)
    store.add_texts(TEXTS, [dict(m) for m in METAS], ids=PKS)
    assert store.delete(ids=[PKS[r] for r in DEAD]).delete_count == len(DEAD)
    bm25 = MI355XBM25Retriever(vectorizer=_Index(), docs=[], k=len(METAS))
    bm25.add_texts(TEXTS, [dict(m) for m in METAS], ids=PKS)
    assert bm25.delete(ids=[PKS[r] for r in DEAD]).delete_count == len(DEAD)
    return store, bm25


@pytest.mark.parametrize("which", range(len(CONDS)))
def test_both_owners_resolve_a_condition_to_the_rows_of_a_walk(owners, which):
    store, bm25 = owners
    conds, want = CONDS[which], brute(CONDS[which])
    assert want or which in (3,)                                                 # only "nowhere.pdf" selects nothing
    for got in (store._filter_rows(conds), bm25._matching(conds)):
        assert got.dtype == np.int64 and got.tolist() == want
    if conds:                                                                    # ... and through the public entry points: filter={field: [values]}
        flt = {f: v for f, v in conds}
        docs = store.similarity_search("record 1", k=len(METAS), filter=flt)
        assert sorted(d.metadata["pk"] for d in docs) == sorted(PKS[r] for r in want)
        if want:
            assert store._index.calls[-1].tolist() == want
        bm25.search_kwargs = {"filter": flt}
        try:
            assert sorted(TEXTS.index(d.page_content) for d in bm25.invoke("q")) == want
        finally:
            bm25.search_kwargs = {}


def test_the_two_spellings_of_the_odd_value_test_agree():
    """`v in vals or v == vals` (kept) against `any(v == x for x in vals) or v == vals` (what the BM25 retriever spelled out), for every
    unhashable value and every value list of the table above -- the same object included, where `in` answers by identity."""
    odd = [m["tags"] for m in METAS if isinstance(m.get("tags"), (list, dict))] + [{"s"}, [[1], {"a": [2]}]]
    lists = [vals for conds in CONDS for _, vals in conds] + [[o] for o in odd] + [odd, [odd[0], "x"]]
    for v in odd:
        for vals in lists + ([v] if isinstance(v, list) else []):               # (the accepted values are always a list)
            assert (v in vals or v == vals) == (any(v == x for x in vals) or v == vals), (v, vals)


# ---- Seqlock ---------------------------------------------------------------------------------------------------------------------------
def _seqlock():
    calls = []
    return Seqlock(threading.RLock(), lambda: calls.append("changed")), calls


def test_a_read_overlapped_by_a_write_is_repeated():
    seq, changed = _seqlock()
    seen = []

    def read():
        seen.append(seq.value)
        if len(seen) == 1:
            with seq.write():
                assert seq.value == 1                                            # odd inside
        return len(seen)
    assert consistent(read, seq) == 2 and seen == [0, 2] and seq.value == 2 and changed == ["changed"]


def test_an_exception_is_the_callers_unless_a_generation_moved():
    seq, _ = _seqlock()
    calls = []

    def fails():
        calls.append(1)
        raise KeyError("row 7")
    with pytest.raises(KeyError):
        consistent(fails, seq)
    assert len(calls) == 1

    def fails_once_renumbered():
        calls.append(2)
        if calls.count(2) == 1:
            with seq.write():
                pass
            raise IndexError("a row number that no longer exists")
        return "second"
    assert consistent(fails_once_renumbered, seq) == "second" and calls.count(2) == 2


def test_consistent_waits_while_a_writer_is_inside():
    seq, _ = _seqlock()
    inside, leave, started, done = (threading.Event() for _ in range(4))
    seen = []

    def writer():
        with seq.write():
            inside.set()
            assert leave.wait(30)

    def read():
        seen.append((seq.value, leave.is_set()))
        return "read"

    def reader():
        started.set()
        seen.append(consistent(read, seq))
        done.set()
    w, r = threading.Thread(target=writer), threading.Thread(target=reader)
    w.start()
    assert inside.wait(30) and seq.value == 1
    r.start()
    assert started.wait(30)
    assert not done.is_set() and seen == []                                      # the writer holds the lock: no read has run
    leave.set()
    w.join(30); r.join(30)
    assert done.is_set() and seen == [(2, True), "read"]


def test_two_seqlocks_repeat_when_only_the_second_moved():
    a, _ = _seqlock()
    b, changed_b = _seqlock()
    seen = []

    def read():
        seen.append((a.value, b.value))
        if len(seen) == 1:
            with b.write():
                pass
        return len(seen)
    assert consistent(read, a, b) == 2 and seen == [(0, 0), (0, 2)] and changed_b == ["changed"]


def test_a_failed_write_section_leaves_the_generation_even_and_reports_the_change():
    seq, changed = _seqlock()
    with pytest.raises(RuntimeError):
        with seq.write():
            assert seq.value == 1 and changed == []
            raise RuntimeError("the index refused")
    assert seq.value == 2 and changed == ["changed"]
    assert consistent(lambda: "ok", seq) == "ok"


# ---- group_conditions -------------------------------------------------------------------------------------------------------------------
def _loops_it_replaced(conds_each):
    """the bookkeeping as the retriever's _search_each wrote it out"""
    plain = [i for i, c in enumerate(conds_each) if c is None]
    keys, conds, q_of = {}, [], []
    for i, c in enumerate(conds_each):
        if c is None:
            continue
        key = repr(c)
        if key not in keys:
            keys[key] = len(conds)
            conds.append(c)
            q_of.append([])
        q_of[keys[key]].append(i)
    return plain, conds, q_of


def _flat_it_replaced(used, q_of):
    return [i for g in used for i in q_of[g]], [n for n, g in enumerate(used) for _ in q_of[g]]


A, B, C = [("source", ["a.pdf"])], [("source", ["b.pdf"]), ("page", [1])], [("pk", ["id-1"])]
GROUP_CASES = [
    [B, None, A, [("source", ["b.pdf"]), ("page", [1])], None, C, [("source", ["a.pdf"])], B],     # first-seen order; equal conditions, distinct objects
    [None, None, None],
    [C, A, C, A],
    [],
]


@pytest.mark.parametrize("which", range(len(GROUP_CASES)))
def test_group_conditions_equals_the_loops_it_replaced(which):
    each = GROUP_CASES[which]
    plain, conds, q_of = group_conditions(each)
    assert (plain, conds, q_of) == _loops_it_replaced(each)
    assert sorted(plain + [i for qs in q_of for i in qs]) == list(range(len(each)))
    for used in (list(range(len(conds))), list(range(len(conds)))[1:], list(range(len(conds)))[::2], []):      # every group, some dropped as empty
        assert flatten_groups([q_of[g] for g in used]) == _flat_it_replaced(used, q_of)
    if which == 0:
        assert plain == [1, 4] and conds == [B, A, C] and q_of == [[0, 3, 7], [2, 6], [5]]
        assert flatten_groups([q_of[0], q_of[2]]) == ([0, 3, 7, 5], [0, 0, 0, 1])


# ---- the module graph -------------------------------------------------------------------------------------------------------------------
def test_bm25_and_records_do_not_import_the_vector_store():
    """In a fresh process.  The package's __init__ imports every public class, the store among them, so it is stood in for by an empty
    package over the same directory: what is checked is what bm25.py and records.py themselves import."""
    code = ("import sys, types; pkg = types.ModuleType('ragmeup_amd'); pkg.__path__ = [%r]; sys.modules['ragmeup_amd'] = pkg\n"
            "import ragmeup_amd.records\n"
            "assert set(m for m in sys.modules if m.startswith('ragmeup_amd.')) == {'ragmeup_amd.records'}, sorted(sys.modules)\n"
            "import ragmeup_amd.bm25\n"
            "assert 'ragmeup_amd.bm25' in sys.modules and 'ragmeup_amd.vectorstore' not in sys.modules\n" % os.path.join(ROOT, "ragmeup_amd"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    src = open(os.path.join(ROOT, "ragmeup_amd", "bm25.py"), encoding="utf-8").read()
    assert "from .vectorstore import" not in src and "import vectorstore" not in src
