"""What the dense store (vectorstore.py) and the BM25 retriever (bm25.py) share about their records: the condition language of
``expr=`` / ``filter=``, the cached field maps that turn a condition into row ids, the seqlock that lets searches run beside a
compaction, and the grouping of one condition per query.  numpy and the standard library only: both owners import this module, it imports
neither."""
from __future__ import annotations

import contextlib
import re
from typing import Any, Callable

import numpy as np

# ---- conditions on records: one language for delete(expr=, filter=) and for every search entry point ------------------------------------
# expr (Milvus style): `field == "v"`, `field in ["a", 'b']`, joined by `and` / `&&`; values are quoted strings or plain numbers.
# filter (PGVector style): {field: value} or {field: [values]} = any of them.  Every condition must hold; "pk" names the primary key.
_EXPR = re.compile(r"""^\s*(\w+)\s*==\s*(['"])(.*)\2\s*$""")        # the whole expression as ONE equality: the value may hold anything
_TOKEN = re.compile(r"""\s*(?:(?P<str>"[^"]*"|'[^']*')|(?P<num>-?\d+(?:\.\d+)?(?![\w.]))|(?P<op>==|&&|\[|\]|,)|(?P<word>\w+))""")


def parse_expr(expr: str) -> list[tuple[str, list]]:
    """-> [(field, [accepted values])]; ValueError for anything the grammar above does not cover (an expression is never ignored)"""
    toks, pos = [], 0
    text = expr.rstrip()
    while pos < len(text):
        m = _TOKEN.match(text, pos)
        if not m:
            toks = None
            break
        kind = m.lastgroup
        raw = m.group(kind)
        toks.append((kind, raw[1:-1] if kind == "str" else (float(raw) if "." in raw else int(raw)) if kind == "num" else raw))
        pos = m.end()
    conds: list[tuple[str, list]] = []

    def value(i):
        if i < len(toks) and toks[i][0] in ("str", "num"):
            return toks[i][1], i + 1
        raise ValueError

    try:
        if not toks:
            raise ValueError
        i = 0
        while True:
            if toks[i][0] != "word" or toks[i][1] in ("and", "in"):
                raise ValueError
            field = toks[i][1]
            if toks[i + 1] == ("op", "=="):
                v, i = value(i + 2)
                conds.append((field, [v]))
            elif toks[i + 1] == ("word", "in") and toks[i + 2] == ("op", "["):
                vals, i = [], i + 3
                while True:
                    v, i = value(i)
                    vals.append(v)
                    if toks[i] == ("op", "]"):
                        i += 1
                        break
                    if toks[i] != ("op", ","):
                        raise ValueError
                    i += 1
                conds.append((field, vals))
            else:
                raise ValueError
            if i == len(toks):
                return conds
            if toks[i] not in (("word", "and"), ("op", "&&")):
                raise ValueError
            i += 1
    except (ValueError, IndexError):
        # what delete() always took: one equality whose value may itself hold quotes -- but not a second condition this grammar
        # does not know (`or`, `>`...): that is an error, not a strange value
        m = _EXPR.match(expr)
        if m and not re.search(r"==|\bin\s*\[", m.group(3)):
            return [(m.group(1), [m.group(3)])]
        raise ValueError(f"unsupported filter expression: {expr!r}") from None


def conditions(expr, filter) -> list[tuple[str, list]] | None:
    """The conditions `expr=` and `filter=` state together, or None when neither is given."""
    if expr is None and filter is None:
        return None
    if filter is not None and not isinstance(filter, dict):
        raise ValueError(f"filter must be a dict of field -> value or list of values, got {type(filter).__name__}")
    if expr is not None and not isinstance(expr, str):
        raise ValueError(f"expr must be a string, got {type(expr).__name__}")
    conds = [(str(f), list(v) if isinstance(v, (list, tuple, set, frozenset)) else [v]) for f, v in (filter or {}).items()]
    if expr is not None and expr.strip():
        conds += parse_expr(expr)
    elif expr is not None and not conds:
        raise ValueError("unsupported filter expression: ''")
    return conds or None                             # (filter={} states nothing)


def conditions_per_query(nq: int, expr, filter, exprs, filters):
    """-> None (no plural form given: the singular expr= / filter= hold for the whole batch, as ever) or a list with one entry per query:
    its conditions, or None for an unfiltered query.  ValueError when a singular and a plural form are given together."""
    if exprs is None and filters is None:
        return None
    if expr is not None or filter is not None:
        raise ValueError("give either expr= / filter= (one condition for the whole batch) or exprs= / filters= (one per query), not both")
    for name, v in (("exprs", exprs), ("filters", filters)):
        if v is not None and (not isinstance(v, (list, tuple)) or len(v) != nq):
            raise ValueError(f"{name} must be a list with one entry per query ({nq}); None = unfiltered")
    return [conditions(exprs[i] if exprs is not None else None, filters[i] if filters is not None else None) for i in range(nq)]


# ---- field maps: a condition is a dictionary look-up, not a walk over the records -------------------------------------------------------
class FieldMaps:
    """field -> (value -> ascending int64 rows of the live records holding it, [(row, value)] of the few records whose value is
    unhashable), built on the first condition that names the field and dropped whenever the owner's records change (``changed``).
    ``lock`` is the owner's writer lock (an RLock).  ``records``, which the owner hands to every call, gives its current (alive, pks,
    metadatas) as parallel sequences; it is called only for a walk, under that lock, so no insert or delete can slip between the walk and
    the cache -- and the maps hold no reference to their owner.  ``builds`` counts the walks."""

    def __init__(self, lock):
        self._lock = lock
        self._maps: dict[str, tuple] = {}
        self.builds = 0

    def changed(self):
        """records were added, removed or renumbered: no map holds any more"""
        self._maps = {}

    def field_map(self, field: str, records: Callable[[], tuple]) -> tuple:
        fm = self._maps.get(field)
        if fm is None:
            with self._lock:
                fm = self._maps.get(field)
                if fm is None:
                    buckets: dict = {}
                    odd: list[tuple[int, Any]] = []
                    alive, pks, metas = records()
                    for r in range(len(alive)):
                        if not alive[r]:
                            continue
                        if field == "pk":
                            v = pks[r]
                        else:
                            v = metas[r].get(field)      # (a record without the field holds None, as delete always compared)
                        try:
                            buckets.setdefault(v, []).append(r)
                        except TypeError:                # a list / dict as metadata value
                            odd.append((r, v))
                    fm = ({v: np.asarray(rs, dtype=np.int64) for v, rs in buckets.items()}, odd)
                    self._maps[field] = fm
                    self.builds += 1
        return fm

    def matching(self, conds, records: Callable[[], tuple]) -> np.ndarray:
        """Ascending int64 rows of the live records that satisfy every condition ("pk" names the primary key); no conditions: all
        live rows (read off ``records()`` without a cached map, so an owner whose ``records`` is costly should not ask this often)."""
        rows = None
        for field, vals in conds or ():
            by_value, odd = self.field_map(field, records)
            parts = []
            for v in vals:
                try:
                    hit = by_value.get(v)
                except TypeError:
                    hit = None
                if hit is not None:
                    parts.append(hit)
            if odd:
                # an odd value matches as an element of `vals` or as the whole list.  `v in vals` is `any(v is x or v == x for x in vals)`;
                # an odd value is a list, dict or set (or another unhashable container), for which identity implies equality, so this is
                # `any(v == x for x in vals)` -- the form the BM25 retriever used to spell out
                parts.append(np.asarray([r for r, v in odd if v in vals or v == vals], dtype=np.int64))
            if not parts:
                return np.zeros(0, np.int64)
            cur = parts[0] if len(parts) == 1 else np.unique(np.concatenate(parts))
            rows = cur if rows is None else np.intersect1d(rows, cur, assume_unique=True)
            if rows.size == 0:
                break
        return rows if rows is not None else np.flatnonzero(np.asarray(records()[0], dtype=bool)).astype(np.int64)


# ---- the seqlock: searches run without the writer lock, a compaction renumbers the rows beside them ------------------------------------
class Seqlock:
    """A generation (``value``) that is odd while the owner renumbers its records under ``lock``.  ``changed`` is the owner's "records
    changed" callback; ``consistent`` is the read side."""

    def __init__(self, lock, changed: Callable[[], None]):
        self.lock, self._changed = lock, changed
        self.value = 0

    @contextlib.contextmanager
    def write(self):
        with self.lock:
            self.value += 1                              # odd: readers that overlap this section repeat their read
            try:
                yield
            finally:
                self._changed()                          # the section renumbered the records (or failed half way)
                self.value += 1


def consistent(read, *seqlocks: Seqlock):
    """Run `read` (index call + row numbers -> Documents) until no write section of any of `seqlocks` overlapped it.  Reads still run in
    parallel with each other; a writer holds its lock while its generation is odd, so waiting on that lock waits for it.  An exception
    out of `read` is swallowed only if a generation moved (e.g. a row number that no longer exists); otherwise it is the caller's."""
    while True:
        gens = [s.value for s in seqlocks]
        if [g for g in gens if g & 1]:                   # (lists, not generators: this runs once per search)
            for s, g in zip(seqlocks, gens):
                if g & 1:
                    with s.lock:
                        pass
            continue
        try:
            out = read()
        except Exception:
            if [s.value for s in seqlocks] != gens:
                continue
            raise
        if [s.value for s in seqlocks] == gens:
            return out


# ---- one condition per query: equal conditions share one list ----------------------------------------------------------------------------
def group_conditions(conds_each: list):
    """-> (the unfiltered queries, the distinct conditions in first-seen order, the queries of each); conditions are equal when their
    repr is."""
    plain, keys, conds, q_of = [], {}, [], []
    for i, c in enumerate(conds_each):
        if c is None:
            plain.append(i)
            continue
        g = keys.setdefault(repr(c), len(conds))
        if g == len(conds):
            conds.append(c)
            q_of.append([])
        q_of[g].append(i)
    return plain, conds, q_of


def flatten_groups(q_of: list) -> tuple[list, list]:
    """The queries of the surviving groups -> (qi, ql): the queries in group order and the group number of each, as the grouped calls
    (search_groups, search_where) take them."""
    return [i for qs in q_of for i in qs], [n for n, qs in enumerate(q_of) for _ in qs]


# ---- small pieces both owners hand out -----------------------------------------------------------------------------------------------------
class DeleteResult(int):
    """int subclass carrying ``delete_count`` (pymilvus MutationResult field read at server.py:385)."""

    def __new__(cls, n: int):
        obj = super().__new__(cls, n)
        obj.delete_count = n
        return obj


def json_default(o):
    """Metadata values loaders produce that JSON does not know (numpy scalars, datetimes, bytes, Paths): stored as plain
    numbers where they are numbers, else as their string form -- persist() must not fail on them."""
    if isinstance(o, np.integer):
        return int(o)
    if isinstance(o, np.floating):
        return float(o)
    if isinstance(o, np.ndarray):
        return o.tolist()
    if isinstance(o, (bytes, bytearray)):
        return o.decode("utf-8", "replace")
    return str(o)
