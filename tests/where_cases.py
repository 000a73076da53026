"""Shared by tests/test_where_cpu.py and tests/test_where_gpu.py: the code rows, the selections and the numpy reference of the device-side
selection (rmu_columns_select / rmu_index_search_where), and the records of the store-level comparison.

Two fields: field 0 holds 7 distinct codes, field 1 holds 300; code 300 of field 1 is held by row 0 alone and code 301 by row n-1 alone
(with n == 1 the one row holds 301).  Every comparison built on these is exact: the lists are sets of integers."""
import hashlib

import numpy as np

N_FIELDS = 2
ROW_COUNTS = (1, 63, 64, 65, 257, 4096, 4097, 70_001)     # 70 001 rows at 64 rows per tile: 1 094 tiles, past a 1 024-wide block scan
ONLY_FIRST, ONLY_LAST = 300, 301


def make_codes(n: int, seed: int = 5) -> np.ndarray:
    rng = np.random.default_rng(seed + n)
    c = np.stack([rng.integers(0, 7, n), rng.integers(0, 300, n)], axis=1).astype(np.int32)
    c[0, 1] = ONLY_FIRST
    c[n - 1, 1] = ONLY_LAST
    return c


def selections():
    """33 selections: [(field, [codes])...] each.  The numbered ones are named in the tests."""
    absent = list(range(1000, 1032))                      # codes no row holds
    sels = [
        [(0, [3])],                                                            # 0: a single code
        [(0, [1, 5])],                                                         # 1: two codes
        [(1, list(range(10, 42)) + absent)],                                   # 2: 64 codes, half of which occur nowhere
        [(1, list(range(0, 300)) + list(range(1000, 1724)))],                  # 3: 1 024 codes: every row but the first and the last
        [(0, [1, 5]), (1, list(range(0, 150)))],                               # 4: two terms
        [(0, [0, 1, 2, 3]), (1, list(range(0, 200))), (0, [1, 2, 3, 6]), (1, list(range(100, 300)))],   # 5: four terms
        [(0, [99])],                                                           # 6: matches nothing
        [(0, list(range(7)))],                                                 # 7: matches every row
        [(1, [ONLY_FIRST])],                                                   # 8: row 0 alone (n > 1)
        [(1, [ONLY_LAST])],                                                    # 9: row n-1 alone
        [(0, [1, 5]), (1, list(range(0, 150)))],                               # 10: identical to 4
        [(0, [5, 6]), (1, list(range(100, 250)))],                             # 11: overlaps 4
        [(0, [2]), (1, [])],                                                   # 12: a term without codes: matches nothing
    ]
    for i in range(len(sels), 33):
        sels.append([(0, [i % 7]), (1, [(37 * i) % 300, (37 * i + 1) % 300, 290])])
    return sels


def reference(codes: np.ndarray, sel) -> np.ndarray:
    """np.flatnonzero of the same predicate: the ascending int64 rows whose codes satisfy every term."""
    keep = np.ones(codes.shape[0], dtype=bool)
    for field, cs in sel:
        keep &= np.isin(codes[:, field], np.asarray(cs, dtype=np.int64))
    return np.flatnonzero(keep).astype(np.int64)


def compact_reference(codes: np.ndarray, dead) -> tuple[np.ndarray, np.ndarray]:
    """-> (old_to_new map as rmu_index_compact returns it, the code rows afterwards)"""
    alive = np.ones(codes.shape[0], dtype=bool)
    alive[np.asarray(dead, dtype=np.int64)] = False
    m = np.where(alive, np.cumsum(alive) - 1, -1).astype(np.int64)
    return m, codes[alive]


# ---- store level ---------------------------------------------------------------------------------------------------------------------
class HashEmbeddings:
    """Unit vectors derived from the text's hash, the same for a document and for a query (the pattern of tests/test_groups_gpu.py)."""

    def __init__(self, dim: int = 384):
        self.dim = dim

    def _vec(self, text):
        seed = int.from_bytes(hashlib.sha256(text.encode()).digest()[:8], "little")
        v = np.random.default_rng(seed).standard_normal(self.dim)
        return (v / np.linalg.norm(v)).astype(np.float32)

    def embed_documents(self, texts):
        return [self._vec(t).tolist() for t in texts]

    def embed_query(self, text):
        return self._vec(text).tolist()


SOURCES = ("a.pdf", "b.pdf", "c.pdf", "d.pdf", "e.pdf", "f.pdf")


def records(n: int = 3000):
    texts = ["chunk %d of the corpus" % i for i in range(n)]
    metas = []
    for i in range(n):
        m = {"source": SOURCES[(i * 7) % len(SOURCES)], "page": i % 5}
        if i % 11:                                       # (every 11th record has no `lang`: it holds None)
            m["lang"] = ("en", "nl", "de")[(i // 3) % 3]
        metas.append(m)
    return texts, metas, ["pk%05d" % i for i in range(n)]


# 17 requests over 5 distinct conditions, one of them None and one matching nothing
_CONDS = ('source == "a.pdf"', 'source in ["b.pdf", "c.pdf"] and lang == "en"', None, 'source == "nowhere.pdf"', 'lang == "nl"')
EXPRS = [_CONDS[i] for i in (0, 1, 2, 3, 4, 0, 0, 1, 4, 2, 1, 0, 4, 4, 3, 1, 0)]
QUERIES = ["request number %d" % i for i in range(len(EXPRS))]
ONE_EXPR = 'source in ["a.pdf", "d.pdf", "zzz.pdf"] and lang == "en"'
