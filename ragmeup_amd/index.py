"""FlatIndex -- Python handle on the HBM-resident flat index behind librmu.so.

Host-side mirror of what the reference reaches through langchain_milvus.Milvus /
langchain_postgres.PGVector (server/RAGHelper.py:385-434, 497-499): insert, exact top-k,
row fetch for MMR, delete.  Arrays are numpy on the host or torch CUDA tensors (device pointers
cross the C-ABI as integers); nothing here computes a score on the CPU.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native as N


def _is_torch_cuda(t) -> bool:
    return hasattr(t, "data_ptr") and hasattr(t, "is_cuda") and bool(t.is_cuda)


def search_groups_blocks(call, q: np.ndarray, k: int, lists, q_list, row_base: int = 0, block: int = N.MAX_QUERIES_PER_CALL):
    """The host half of FlatIndex.search_groups, a pure function of its arguments: sort the queries by list (stable), cut them into blocks
    of at most `block`, hand each block to `call(q_block, k, rows, list_ptr, q_list_block, row_base) -> (scores, rows)` with ONLY the lists
    that block uses (laid end to end, list_ptr rebased to 0, q_list_block non-decreasing int32), and put the results back in the caller's
    order."""
    n_lists = len(lists)
    ql = np.asarray(q_list, dtype=np.int64).reshape(-1)
    nq = q.shape[0]
    if ql.shape[0] != nq:
        raise ValueError(f"q_list names the list of each query: expected {nq} entries, got {ql.shape[0]}")
    if nq and (n_lists == 0 or ql.min() < 0 or ql.max() >= n_lists):
        raise ValueError(f"q_list entries must be in [0, {n_lists})")
    on_device = n_lists > 0 and all(_is_torch_cuda(x) for x in lists)
    if on_device:
        import torch
        if any(x.dtype != torch.int64 or x.ndim != 1 for x in lists):
            raise ValueError("device lists must be 1-d int64 tensors")
        lens = [int(x.shape[0]) for x in lists]
    else:
        if any(_is_torch_cuda(x) for x in lists):
            raise ValueError("the lists must be all host arrays or all device tensors")
        lists = [np.ascontiguousarray(x, dtype=np.int64).reshape(-1) for x in lists]
        lens = [int(x.shape[0]) for x in lists]
    ptr = np.zeros(n_lists + 1, dtype=np.int64)
    np.cumsum(lens, out=ptr[1:])
    order = np.argsort(ql, kind="stable")
    out_s = np.empty((nq, k), dtype=np.float32)
    out_r = np.empty((nq, k), dtype=np.int64)
    for b0 in range(0, nq, block):
        sel = order[b0:b0 + block]
        lo, hi = int(ql[sel[0]]), int(ql[sel[-1]]) + 1        # the lists of this block: a contiguous range, the queries are sorted
        if on_device:
            rows = torch.cat(list(lists[lo:hi])).contiguous()
            torch.cuda.current_stream().synchronize()
        else:
            rows = np.concatenate(lists[lo:hi]) if hi > lo else np.empty(0, np.int64)
        s, r = call(np.ascontiguousarray(q[sel]), k, rows, np.ascontiguousarray(ptr[lo:hi + 1] - ptr[lo]), (ql[sel] - lo).astype(np.int32), row_base)
        out_s[sel], out_r[sel] = s, r
    return out_s, out_r


def flatten_selections(selections):
    """[[(field_no, [codes...]), ...], ...] -> (terms int32 [n_terms, 3] = field, codes_begin, codes_end; codes int32; sel_ptr int32
    [n_sel + 1]): the flattened form rmu_columns_select takes.  The codes of a term are deduplicated and sorted here; everything else
    (field numbers, term and code counts) is the library's to check."""
    terms, codes, sel_ptr = [], [], [0]
    for sel in selections:
        for field, cs in sel:
            cs = np.unique(np.asarray(list(cs), dtype=np.int64))
            if cs.size and (cs[0] < 0 or cs[-1] > 0x7FFFFFFF):
                raise ValueError("codes must be in [0, 2^31)")
            terms.append((int(field), len(codes), len(codes) + int(cs.size)))
            codes.extend(cs.tolist())
        sel_ptr.append(len(terms))
    return (np.asarray(terms, dtype=np.int32).reshape(-1, 3), np.asarray(codes, dtype=np.int32), np.asarray(sel_ptr, dtype=np.int32))


class Columns:
    """Metadata columns of a FlatIndex (rmu_columns_*): one int32 code per row and field, numbered by the caller.  The master copy is on the
    host (append, compact and len never touch the GPU); the device image follows at the next selection."""

    def __init__(self, n_fields: int, capacity_hint: int = 0):
        self._lib = N.lib()
        self.n_fields = int(n_fields)
        h = ctypes.c_void_p()
        N.check(self._lib.rmu_columns_create(ctypes.byref(h), self.n_fields, int(capacity_hint)), "rmu_columns_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.rmu_columns_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self) -> int:
        n = ctypes.c_int64()
        N.check(self._lib.rmu_columns_size(self._h, ctypes.byref(n), None), "rmu_columns_size")
        return int(n.value)

    def append(self, codes) -> int:
        """codes [n, n_fields] (or [n] for one field), every code >= 0; returns the row of codes[0]."""
        c = np.ascontiguousarray(codes, dtype=np.int32)
        if c.ndim == 1 and self.n_fields == 1:
            c = c[:, None]
        if c.ndim != 2 or c.shape[1] != self.n_fields:
            raise ValueError(f"expected [n, {self.n_fields}] got {c.shape}")
        first = ctypes.c_int64()
        N.check(self._lib.rmu_columns_append(self._h, c.ctypes.data, c.shape[0], ctypes.byref(first)), "rmu_columns_append")
        return int(first.value)

    def compact(self, old_to_new) -> int:
        """Apply the map FlatIndex.compact() returned; returns the rows afterwards."""
        m = np.ascontiguousarray(old_to_new, dtype=np.int64).reshape(-1)
        after = ctypes.c_int64()
        N.check(self._lib.rmu_columns_compact(self._h, m.ctypes.data, m.shape[0], ctypes.byref(after)), "rmu_columns_compact")
        return int(after.value)

    def set_tile_rows(self, rows: int = 0):
        """RMU_COLUMNS_OPT_TILE_ROWS (testing switch): a power of two in [64, 16384], 0 = default; results are identical for every value."""
        N.check(self._lib.rmu_columns_set_option(self._h, N.COLUMNS_OPT_TILE_ROWS, int(rows)), "rmu_columns_set_option")

    def select(self, selections, count_only: bool = False, device: bool = False):
        """selections: [[(field_no, [codes...]), ...], ...] -> one ascending int64 row array per selection (numpy; `device`: views of one
        torch CUDA tensor).  count_only: the int64 list_ptr [n_sel + 1] instead.  A convenience for tests and tools, not a hot path: it
        calls the library twice -- once to count, so that the output can be allocated, once for the lists -- and so runs the count pass
        twice; FlatIndex.search_where is the one-call form."""
        terms, codes, sel_ptr = flatten_selections(selections)
        n_sel = len(sel_ptr) - 1
        lp = np.zeros(n_sel + 1, dtype=np.int64)

        def call(flags, out_ptr, cap):
            return self._lib.rmu_columns_select(self._h, terms.ctypes.data, terms.shape[0], codes.ctypes.data, sel_ptr.ctypes.data, n_sel,
                                                flags, out_ptr, cap, lp.ctypes.data, 0)
        N.check(call(0, None, 0), "rmu_columns_select")
        if count_only:
            return lp
        total = int(lp[-1])
        if device:
            import torch
            out = torch.empty(max(total, 1), dtype=torch.int64, device="cuda")
            torch.cuda.current_stream().synchronize()
            N.check(call(N.F_OUT_DEVICE, out.data_ptr(), total), "rmu_columns_select")
        else:
            out = np.empty(max(total, 1), dtype=np.int64)
            N.check(call(0, out.ctypes.data, total), "rmu_columns_select")
        return [out[int(lp[g]):int(lp[g + 1])] for g in range(n_sel)]


class FlatIndex:
    def __init__(self, dim: int, metric: int = N.METRIC_IP, capacity_hint: int = 0, device: int | None = None):
        """dim <= 3072 (N.MAX_DIM_WIDE) for METRIC_IP / METRIC_COSINE, <= 767 for METRIC_L2SQ; RmuError otherwise."""
        self._lib = N.lib()
        if device is not None:
            N.check(self._lib.rmu_init(int(device)), "rmu_init")
        self.dim = int(dim)
        self.metric = int(metric)
        h = ctypes.c_void_p()
        N.check(self._lib.rmu_index_create(ctypes.byref(h), self.dim, self.metric, int(capacity_hint)),
                "rmu_index_create")
        self._h = h

    # -- persistence ---------------------------------------------------------------------
    def save(self, path: str):
        N.check(self._lib.rmu_index_save(self._h, str(path).encode()), "rmu_index_save")

    @classmethod
    def load(cls, path: str, device: int | None = None) -> "FlatIndex":
        self = cls.__new__(cls)
        self._lib = N.lib()
        if device is not None:
            N.check(self._lib.rmu_init(int(device)), "rmu_init")
        h = ctypes.c_void_p()
        N.check(self._lib.rmu_index_load(ctypes.byref(h), str(path).encode()), "rmu_index_load")
        self._h = h
        d = ctypes.c_int()
        N.check(self._lib.rmu_index_dim(h, ctypes.byref(d)), "rmu_index_dim")
        self.dim = int(d.value)
        m = ctypes.c_int()
        N.check(self._lib.rmu_index_metric(h, ctypes.byref(m)), "rmu_index_metric")
        self.metric = int(m.value)                 # what the file header says, not an assumption
        return self

    # -- lifecycle ---------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._lib.rmu_index_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self) -> int:
        n = ctypes.c_int64()
        N.check(self._lib.rmu_index_size(self._h, ctypes.byref(n)), "rmu_index_size")
        return int(n.value)

    def stats(self) -> dict:
        """rmu_index_stat: allocated capacity, re-allocations by add() and their wall time, live rows."""
        out = {}
        for name, what in (("capacity", N.STAT_CAPACITY), ("grow_count", N.STAT_GROW_COUNT), ("grow_ms", N.STAT_GROW_MS),
                           ("live_rows", N.STAT_LIVE_ROWS)):
            v = ctypes.c_double()
            N.check(self._lib.rmu_index_stat(self._h, what, ctypes.byref(v)), "rmu_index_stat")
            out[name] = float(v.value) if name == "grow_ms" else int(v.value)
        return out

    def compaction_stats(self) -> dict:
        """rmu_index_stat: how many compact() calls dropped rows, and their wall time."""
        out = {}
        for name, what in (("compact_count", N.STAT_COMPACT_COUNT), ("compact_ms", N.STAT_COMPACT_MS)):
            v = ctypes.c_double()
            N.check(self._lib.rmu_index_stat(self._h, what, ctypes.byref(v)), "rmu_index_stat")
            out[name] = float(v.value) if name == "compact_ms" else int(v.value)
        return out

    def reserve(self, rows: int):
        """Make room for `rows` rows in all (grow-only; see rmu_index_reserve): a re-allocation waits for the device, so a caller that is
        about to leave work in flight does it first."""
        N.check(self._lib.rmu_index_reserve(self._h, int(rows)), "rmu_index_reserve")

    # -- mutation ----------------------------------------------------------------------------------
    def add(self, vecs) -> int:
        """Append rows; returns the row id of the first one."""
        first = ctypes.c_int64()
        if _is_torch_cuda(vecs):
            import torch
            v = vecs.detach().to(torch.float32).contiguous()
            if v.ndim != 2 or v.shape[1] != self.dim:
                raise ValueError(f"expected [n, {self.dim}] got {tuple(v.shape)}")
            torch.cuda.current_stream().synchronize()
            N.check(self._lib.rmu_index_add(self._h, v.data_ptr(), v.shape[0], 1, ctypes.byref(first)), "rmu_index_add")
        else:
            v = np.ascontiguousarray(vecs, dtype=np.float32)
            if v.ndim != 2 or v.shape[1] != self.dim:
                raise ValueError(f"expected [n, {self.dim}] got {v.shape}")
            N.check(self._lib.rmu_index_add(self._h, v.ctypes.data, v.shape[0], 0, ctypes.byref(first)), "rmu_index_add")
        return int(first.value)

    def remove_rows(self, rows) -> int:
        r = np.ascontiguousarray(rows, dtype=np.int64)
        cnt = ctypes.c_int64()
        N.check(self._lib.rmu_index_remove_rows(self._h, r.ctypes.data, r.shape[0], ctypes.byref(cnt)),
                "rmu_index_remove_rows")
        return int(cnt.value)

    def compact(self) -> np.ndarray:
        """Drop the tombstoned rows (rmu_index_compact): live rows keep their order and become rows 0..n_live-1.  Returns the int64 map
        old row -> new row (-1 = the row was dead), one entry per row the index held."""
        after = ctypes.c_int64()
        while True:
            n = len(self)
            m = np.empty(max(n, 1), dtype=np.int64)
            rc = self._lib.rmu_index_compact(self._h, m.ctypes.data, n, ctypes.byref(after))
            if rc != N.RMU_OK and len(self) > n:         # rows were added between the size and the call: a longer map
                continue
            N.check(rc, "rmu_index_compact")
            return m[:n]

    def set_compact_inplace(self, on: bool = True):
        """RMU_OPT_COMPACT_INPLACE: compact() moves rows inside the current allocations (capacity kept) instead of into smaller ones;
        results are identical either way."""
        N.check(self._lib.rmu_index_set_option(self._h, N.OPT_COMPACT_INPLACE, 1 if on else 0), "rmu_index_set_option")

    def get_rows(self, rows) -> np.ndarray:
        r = np.ascontiguousarray(rows, dtype=np.int64)
        out = np.empty((r.shape[0], self.dim), dtype=np.float32)
        N.check(self._lib.rmu_index_get_rows(self._h, r.ctypes.data, r.shape[0], out.ctypes.data), "rmu_index_get_rows")
        return out

    def mmr(self, q, rows, k: int, lambda_mult: float = 0.5) -> np.ndarray:
        """Batched greedy MMR on the device: q [nq, dim] fp32, rows [nq, fetch_k] int64 candidate row ids (-1 = absent, as
        `search` pads them; without a row_base) -> positions [nq, k] int32 into each candidate list (-1 = none).  An id past the last row and
        the id of a removed row (a list from before a `remove_rows`) are absent as well."""
        qq = np.ascontiguousarray(q, dtype=np.float32)
        if qq.ndim == 1:
            qq = qq[None]
        r = np.ascontiguousarray(rows, dtype=np.int64)
        if r.ndim == 1:
            r = r[None]
        if r.shape[0] != qq.shape[0] or qq.shape[1] != self.dim:
            raise ValueError("mmr: q must be [nq, dim] and rows [nq, fetch_k]")
        out = np.empty((qq.shape[0], int(k)), dtype=np.int32)
        N.check(self._lib.rmu_index_mmr(self._h, qq.ctypes.data, qq.shape[0], r.ctypes.data, r.shape[1], int(k),
                                        float(lambda_mult), 0, out.ctypes.data), "rmu_index_mmr")
        return out

    def search_mmr(self, q, fetch_k: int, k: int, lambda_mult: float = 0.5, row_base: int = 0):
        """`search(q, fetch_k)` + `mmr(...)` in one call with one host round trip (rmu_index_search_mmr; the reference's per-request
        retriever call): q [nq, dim] host fp32 -> (rows [nq, k] int64 in pick order, -1 padded; scores [nq, k] fp32)."""
        qq = np.ascontiguousarray(q, dtype=np.float32)
        if qq.ndim == 1:
            qq = qq[None]
        if qq.shape[1] != self.dim:
            raise ValueError(f"expected [nq, {self.dim}] got {qq.shape}")
        nq = qq.shape[0]
        rows = np.empty((nq, int(k)), dtype=np.int64)
        scores = np.empty((nq, int(k)), dtype=np.float32)
        N.check(self._lib.rmu_index_search_mmr(self._h, qq.ctypes.data, nq, int(fetch_k), int(k), float(lambda_mult), int(row_base),
                                               rows.ctypes.data, scores.ctypes.data), "rmu_index_search_mmr")
        return rows, scores

    # -- search ------------------------------------------------------------------------------------
    def search(self, q, k: int, row_base: int = 0, stream: int | None = None, out=None, rows=None):
        """Exact top-k.  numpy in -> numpy out; torch CUDA in -> torch CUDA out (same device).
        `stream` (torch CUDA input only): a non-zero hipStream_t handle (`torch.cuda.Stream.cuda_stream`) the search is ORDERED
        on -- the call returns without any host synchronisation (include/rmu.h stream contract) and the outputs are valid for
        work queued behind it on that stream.  Default: complete on return.
        `rows`: search these rows only (rmu_index_search_subset: a gathered scan, time proportional to the list) -- strictly ascending
        index-local row ids, one list for all queries: a numpy int64 array (checked: RmuError RMU_E_INVALID when not ascending or out of
        range) or, with torch CUDA queries, a torch CUDA int64 tensor (not checked: ids outside the index are ignored).  Scores and
        order are those `search` without `rows` gives the same rows; fewer than k live rows in the list: (-inf | +inf, -1) padding.
        ValueError on an index of more than 768 dimensions (N.MAX_DIM): the wide scan has no gathered form yet."""
        if rows is not None:
            return self._search_subset(q, int(k), int(row_base), stream, out, rows)
        if _is_torch_cuda(q):
            import torch
            qq = q.detach().to(torch.float32).contiguous()
            if qq.ndim == 1:
                qq = qq[None]
            nq = qq.shape[0]
            if out is not None:                  # caller-owned result tensors (a serving loop's)
                out_s, out_r = out
                if (out_s.shape != (nq, k) or out_r.shape != (nq, k) or out_s.dtype != torch.float32 or out_r.dtype != torch.int64
                        or not out_s.is_contiguous() or not out_r.is_contiguous() or out_s.device != qq.device or out_r.device != qq.device):
                    raise ValueError("out must be (float32 [nq, k], int64 [nq, k]) contiguous tensors on the queries' device")
            else:
                out_s = torch.empty((nq, k), dtype=torch.float32, device=qq.device)
                out_r = torch.empty((nq, k), dtype=torch.int64, device=qq.device)
            if not stream:
                torch.cuda.current_stream().synchronize()
            N.check(self._lib.rmu_index_search(self._h, qq.data_ptr(), nq, int(k), N.F_Q_DEVICE | N.F_OUT_DEVICE,
                                               int(row_base), out_s.data_ptr(), out_r.data_ptr(), int(stream or 0)),
                    "rmu_index_search")
            return out_s, out_r
        qq = np.ascontiguousarray(q, dtype=np.float32)
        if qq.ndim == 1:
            qq = qq[None]
        if qq.shape[1] != self.dim:
            raise ValueError(f"expected [nq, {self.dim}] got {qq.shape}")
        nq = qq.shape[0]
        out_s = np.empty((nq, k), dtype=np.float32)
        out_r = np.empty((nq, k), dtype=np.int64)
        N.check(self._lib.rmu_index_search(self._h, qq.ctypes.data, nq, int(k), 0, int(row_base),
                                           out_s.ctypes.data, out_r.ctypes.data, 0), "rmu_index_search")
        return out_s, out_r

    def _search_subset(self, q, k: int, row_base: int, stream, out, rows):
        if self.dim > N.MAX_DIM:
            raise ValueError(f"search(rows=...) serves rows of at most {N.MAX_DIM} dimensions; this index holds {self.dim}-d rows "
                             "(the filtered search of a wide index does not exist yet)")
        if _is_torch_cuda(q):
            import torch
            qq = q.detach().to(torch.float32).contiguous()
            if qq.ndim == 1:
                qq = qq[None]
            if qq.shape[1] != self.dim:
                raise ValueError(f"expected [nq, {self.dim}] got {tuple(qq.shape)}")
            nq = qq.shape[0]
            flags = N.F_Q_DEVICE | N.F_OUT_DEVICE
            if _is_torch_cuda(rows):
                if rows.dtype != torch.int64 or rows.ndim != 1 or rows.device != qq.device:
                    raise ValueError("rows must be a 1-d int64 tensor on the queries' device")
                rr = rows.contiguous()
                rows_ptr, n_sub = rr.data_ptr(), int(rr.shape[0])
                flags |= N.F_ROWS_DEVICE
            else:
                rr = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
                rows_ptr, n_sub = rr.ctypes.data, int(rr.shape[0])
            if out is not None:
                out_s, out_r = out
                if (out_s.shape != (nq, k) or out_r.shape != (nq, k) or out_s.dtype != torch.float32 or out_r.dtype != torch.int64
                        or not out_s.is_contiguous() or not out_r.is_contiguous() or out_s.device != qq.device or out_r.device != qq.device):
                    raise ValueError("out must be (float32 [nq, k], int64 [nq, k]) contiguous tensors on the queries' device")
            else:
                out_s = torch.empty((nq, k), dtype=torch.float32, device=qq.device)
                out_r = torch.empty((nq, k), dtype=torch.int64, device=qq.device)
            if not stream:
                torch.cuda.current_stream().synchronize()
            N.check(self._lib.rmu_index_search_subset(self._h, qq.data_ptr(), nq, k, flags, row_base, rows_ptr, n_sub,
                                                      out_s.data_ptr(), out_r.data_ptr(), int(stream or 0)), "rmu_index_search_subset")
            return out_s, out_r
        if _is_torch_cuda(rows):
            raise ValueError("a device row list needs device queries")
        qq = np.ascontiguousarray(q, dtype=np.float32)
        if qq.ndim == 1:
            qq = qq[None]
        if qq.shape[1] != self.dim:
            raise ValueError(f"expected [nq, {self.dim}] got {qq.shape}")
        rr = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        nq = qq.shape[0]
        out_s = np.empty((nq, k), dtype=np.float32)
        out_r = np.empty((nq, k), dtype=np.int64)
        N.check(self._lib.rmu_index_search_subset(self._h, qq.ctypes.data, nq, k, 0, row_base, rr.ctypes.data, int(rr.shape[0]),
                                                  out_s.ctypes.data, out_r.ctypes.data, 0), "rmu_index_search_subset")
        return out_s, out_r

    def search_groups(self, q, k: int, lists, q_list, row_base: int = 0):
        """Exact top-k of every query against ITS OWN list of rows, all in one scan (rmu_index_search_groups): `lists` is a sequence of
        strictly ascending int64 row-id arrays (they may overlap, repeat each other, be empty or go unused), `q_list[i]` the list of
        query i, in any order.  numpy in -> numpy out: for query i exactly what `search(q[i], k, rows=lists[q_list[i]])` returns.  The
        queries are sorted by list (stably), sent in blocks of at most N.MAX_QUERIES_PER_CALL and put back in the caller's order.
        The lists may also ALL be torch CUDA int64 tensors: they reach the library as a device array, which is not checked (ids outside
        the index are ignored)."""
        if self.dim > N.MAX_DIM:
            raise ValueError(f"search_groups serves rows of at most {N.MAX_DIM} dimensions; this index holds {self.dim}-d rows "
                             "(the filtered search of a wide index does not exist yet)")
        qq = np.ascontiguousarray(q, dtype=np.float32)
        if qq.ndim == 1:
            qq = qq[None]
        if qq.shape[1] != self.dim:
            raise ValueError(f"expected [nq, {self.dim}] got {qq.shape}")
        return search_groups_blocks(self._groups_call, qq, int(k), lists, q_list, int(row_base))

    def _groups_call(self, qq: np.ndarray, k: int, rows, list_ptr: np.ndarray, q_list: np.ndarray, row_base: int):
        """One rmu_index_search_groups call: qq [nq <= 8192, dim] float32, rows = the lists end to end (numpy int64, or a torch CUDA int64
        tensor), list_ptr int64 [n_lists + 1], q_list int32 [nq] non-decreasing."""
        nq = qq.shape[0]
        out_s = np.empty((nq, k), dtype=np.float32)
        out_r = np.empty((nq, k), dtype=np.int64)
        flags, rows_ptr = (N.F_ROWS_DEVICE, rows.data_ptr()) if _is_torch_cuda(rows) else (0, rows.ctypes.data)
        N.check(self._lib.rmu_index_search_groups(self._h, qq.ctypes.data, nq, k, flags, row_base, rows_ptr, list_ptr.ctypes.data,
                                                  int(list_ptr.shape[0]) - 1, q_list.ctypes.data, out_s.ctypes.data, out_r.ctypes.data, 0),
                "rmu_index_search_groups")
        return out_s, out_r

    def search_where(self, q, k: int, columns: "Columns", selections, q_sel, row_base: int = 0):
        """Exact top-k of every query against the rows ITS SELECTION names, the lists built on the device (rmu_index_search_where):
        `selections` is a sequence of [(field_no, [codes...]), ...] conjunctions over `columns`, `q_sel[i]` the selection of query i, in
        any order.  numpy in -> numpy out: for query i exactly what `search(q[i], k, rows=<the rows of its selection>)` returns.  The
        queries are sorted by selection (stably), sent in blocks of at most N.MAX_QUERIES_PER_CALL -- each with only the selections it names --
        and put back in the caller's order.  The codes of a term are deduplicated and sorted here."""
        if self.dim > N.MAX_DIM:
            raise ValueError(f"search_where serves rows of at most {N.MAX_DIM} dimensions; this index holds {self.dim}-d rows "
                             "(the filtered search of a wide index does not exist yet)")
        qq = np.ascontiguousarray(q, dtype=np.float32)
        if qq.ndim == 1:
            qq = qq[None]
        if qq.shape[1] != self.dim:
            raise ValueError(f"expected [nq, {self.dim}] got {qq.shape}")
        k = int(k)
        selections = list(selections)
        nq, n_sel = qq.shape[0], len(selections)
        qs = np.asarray(q_sel, dtype=np.int64).reshape(-1)
        if qs.shape[0] != nq:
            raise ValueError(f"q_sel names the selection of each query: expected {nq} entries, got {qs.shape[0]}")
        if nq and (n_sel == 0 or qs.min() < 0 or qs.max() >= n_sel):
            raise ValueError(f"q_sel entries must be in [0, {n_sel})")
        order = np.argsort(qs, kind="stable")
        out_s = np.empty((nq, k), dtype=np.float32)
        out_r = np.empty((nq, k), dtype=np.int64)
        for b0 in range(0, nq, N.MAX_QUERIES_PER_CALL):
            pick = order[b0:b0 + N.MAX_QUERIES_PER_CALL]
            named, ql = np.unique(qs[pick], return_inverse=True)  # only the selections this block names, renumbered (the queries are sorted)
            terms, codes, sel_ptr = flatten_selections([selections[int(g)] for g in named])
            qb = np.ascontiguousarray(qq[pick])
            ql = ql.astype(np.int32)
            s = np.empty((len(pick), k), dtype=np.float32)
            r = np.empty((len(pick), k), dtype=np.int64)
            N.check(self._lib.rmu_index_search_where(self._h, columns._h, qb.ctypes.data, len(pick), k, 0, int(row_base), terms.ctypes.data,
                                                     terms.shape[0], codes.ctypes.data, sel_ptr.ctypes.data, len(named), ql.ctypes.data,
                                                     s.ctypes.data, r.ctypes.data, 0), "rmu_index_search_where")
            out_s[pick], out_r[pick] = s, r
        return out_s, out_r

    def search_distinct(self, q, k: int, columns: "Columns", field: int, row_base: int = 0):
        """Grouped exact top-k (rmu_index_search_distinct): the best row of each of the k best groups, a group being the rows that share
        one code in column `field` of `columns` (which must hold as many rows as the index).  -> (scores, rows) [nq, k]: the rows `search`
        would return, in its order, with every row dropped whose group an earlier row already represents; each score has the bits
        `search` gives that row; fewer than k live groups: (-inf | +inf, -1) padding.  numpy in -> numpy out; torch CUDA in -> torch
        CUDA out.  k <= N.MAX_K_DISTINCT.  ValueError on an index of more than 768 dimensions (N.MAX_DIM): a wide index is not served."""
        if self.dim > N.MAX_DIM:
            raise ValueError(f"search_distinct serves rows of at most {N.MAX_DIM} dimensions; this index holds {self.dim}-d rows "
                             "(the grouped search of a wide index does not exist)")
        k = int(k)
        if _is_torch_cuda(q):
            import torch
            qq = q.detach().to(torch.float32).contiguous()
            if qq.ndim == 1:
                qq = qq[None]
            if qq.shape[1] != self.dim:
                raise ValueError(f"expected [nq, {self.dim}] got {tuple(qq.shape)}")
            nq = qq.shape[0]
            out_s = torch.empty((nq, k), dtype=torch.float32, device=qq.device)
            out_r = torch.empty((nq, k), dtype=torch.int64, device=qq.device)
            torch.cuda.current_stream().synchronize()
            N.check(self._lib.rmu_index_search_distinct(self._h, columns._h, int(field), qq.data_ptr(), nq, k, N.F_Q_DEVICE | N.F_OUT_DEVICE,
                                                        int(row_base), out_s.data_ptr(), out_r.data_ptr(), 0), "rmu_index_search_distinct")
            return out_s, out_r
        qq = np.ascontiguousarray(q, dtype=np.float32)
        if qq.ndim == 1:
            qq = qq[None]
        if qq.shape[1] != self.dim:
            raise ValueError(f"expected [nq, {self.dim}] got {qq.shape}")
        nq = qq.shape[0]
        out_s = np.empty((nq, k), dtype=np.float32)
        out_r = np.empty((nq, k), dtype=np.int64)
        N.check(self._lib.rmu_index_search_distinct(self._h, columns._h, int(field), qq.ctypes.data, nq, k, 0, int(row_base),
                                                    out_s.ctypes.data, out_r.ctypes.data, 0), "rmu_index_search_distinct")
        return out_s, out_r

    def set_screening(self, on: bool = True):
        """RMU_OPT_SCREEN: allow (default) or forbid the fp16 screening path; results are identical either way."""
        N.check(self._lib.rmu_index_set_option(self._h, N.OPT_SCREEN, 1 if on else 0), "rmu_index_set_option")

    def set_wide_scan(self, on: bool = True):
        """RMU_OPT_WIDE_SCAN (ip / cosine): exact searches run scan_wide_kernel -- the kernel of rows wider than 768 dimensions, which streams
        its queries -- whatever the width, and the screening path is off; results are identical either way, bit for bit."""
        N.check(self._lib.rmu_index_set_option(self._h, N.OPT_WIDE_SCAN, 1 if on else 0), "rmu_index_set_option")

    def set_screen_min_batch(self, n: int = 0):
        """RMU_OPT_SCREEN_MIN_NQ: n > 0 sends every batch of >= n queries through the screening path whatever the corpus size
        (0 restores the default heuristics); results are identical either way."""
        N.check(self._lib.rmu_index_set_option(self._h, N.OPT_SCREEN_MIN_NQ, int(n)), "rmu_index_set_option")

    def set_ladder(self, ratio: int = 0, first: int = 0):
        """Tuning (RMU_OPT_LADDER_RATIO / RMU_OPT_LADDER_FIRST): geometry of the screening path's threshold ladder -- growth ratio above
        64k rows and the size of the first range; 0 = the defaults.  Results are identical for every value (tools/ladder_sweep.py)."""
        N.check(self._lib.rmu_index_set_option(self._h, N.OPT_LADDER_RATIO, int(ratio)), "rmu_index_set_option")
        N.check(self._lib.rmu_index_set_option(self._h, N.OPT_LADDER_FIRST, int(first)), "rmu_index_set_option")

    def set_screen_band(self, on: bool = True):
        """Tuning (RMU_OPT_SCREEN_BAND): the ladder's merges seed each launch's thresholds with max(K'-th best, k-th best - 2 EPS(q)) (default)
        or with the K'-th best alone.  Results and re-run counts are identical either way."""
        N.check(self._lib.rmu_index_set_option(self._h, N.OPT_SCREEN_BAND, 1 if on else 0), "rmu_index_set_option")

    def set_screen_spill(self, on: bool = True, cap: int = 0):
        """Tuning (RMU_OPT_SCREEN_SPILL / RMU_OPT_SCREEN_SPILL_CAP): the seeded launches of a full batch's ladder write passing scores out as they
        are and a sift kernel files them behind the launch (default), or append them inside the scan's tile loop as before; `cap` = records
        per spill list (0 = the default), a full list sends its wave back to appending.  Results and re-run counts are identical either way."""
        N.check(self._lib.rmu_index_set_option(self._h, N.OPT_SCREEN_SPILL, 1 if on else 0), "rmu_index_set_option")
        N.check(self._lib.rmu_index_set_option(self._h, N.OPT_SCREEN_SPILL_CAP, int(cap)), "rmu_index_set_option")

    def set_screen_refresh(self, on: bool = False):
        """Tuning (RMU_OPT_SCREEN_REFRESH): in a spill launch only the waves that can use their queries' shared thresholds re-read them
        (default), or every wave re-reads and refreshes them at every pair of tiles.  Results and re-run counts are identical either way."""
        N.check(self._lib.rmu_index_set_option(self._h, N.OPT_SCREEN_REFRESH, 1 if on else 0), "rmu_index_set_option")

    def screen_candidates(self, q):
        """Test hook (rmu_index_screen_candidates): per query the screening pass's 32 candidates ->
        (approx scores [nq,32], rows [nq,32], exact fp32 scores of the same rows [nq,32], EPS [nq])."""
        qq = np.ascontiguousarray(q, dtype=np.float32)
        if qq.ndim == 1:
            qq = qq[None]
        nq = qq.shape[0]
        ap = np.empty((nq, 32), np.float32)
        ro = np.empty((nq, 32), np.int64)
        ex = np.empty((nq, 32), np.float32)
        eps = np.empty((nq,), np.float32)
        N.check(self._lib.rmu_index_screen_candidates(self._h, qq.ctypes.data, nq, ap.ctypes.data, ro.ctypes.data, ex.ctypes.data,
                                                      eps.ctypes.data), "rmu_index_screen_candidates")
        return ap, ro, ex, eps

    # -- measurement hooks (bench.py) ----------------------------------------------------------------
    def set_timing(self, on: bool = True):
        self._lib.rmu_set_timing(1 if on else 0)

    def last_scan_ms(self) -> float:
        return float(self._lib.rmu_last_scan_ms())

    def last_search_ms(self) -> float:
        return float(self._lib.rmu_last_search_ms())

    def last_screened(self) -> int:
        """>0: answered by the fp16 screening pass + exact re-score; 0: exact scan; <0: screened, with that many queries
        re-run on the exact scan."""
        return int(self._lib.rmu_last_screened())

    def last_geometry(self) -> dict:
        g, b, l, p = (ctypes.c_int() for _ in range(4))
        self._lib.rmu_last_scan_geometry(ctypes.byref(g), ctypes.byref(b), ctypes.byref(l), ctypes.byref(p))
        return {"grid": g.value, "block": b.value, "lds_bytes": l.value, "launches": p.value}


def topk_merge(part_scores, part_rows, k: int | None = None, smaller_better: bool = False, stream: int | None = None):
    """Merge [parts, nq, k] shard lists (numpy or torch CUDA) -> [nq, k].  smaller_better: the scores are distances
    (lists of an RMU_METRIC_L2SQ index).  `stream` as in FlatIndex.search (torch CUDA lists only)."""
    lib = N.lib()
    fl = N.F_SMALLER_BETTER if smaller_better else 0
    if _is_torch_cuda(part_scores):
        import torch
        s = part_scores.detach().to(torch.float32).contiguous()
        r = part_rows.detach().to(torch.int64).contiguous()
        parts, nq, kk = s.shape
        out_s = torch.empty((nq, kk), dtype=torch.float32, device=s.device)
        out_r = torch.empty((nq, kk), dtype=torch.int64, device=s.device)
        if not stream:
            torch.cuda.current_stream().synchronize()
        N.check(lib.rmu_topk_merge(s.data_ptr(), r.data_ptr(), parts, nq, kk, N.F_Q_DEVICE | N.F_OUT_DEVICE | fl,
                                   out_s.data_ptr(), out_r.data_ptr(), int(stream or 0)), "rmu_topk_merge")
        return out_s, out_r
    s = np.ascontiguousarray(part_scores, dtype=np.float32)
    r = np.ascontiguousarray(part_rows, dtype=np.int64)
    parts, nq, kk = s.shape
    out_s = np.empty((nq, kk), dtype=np.float32)
    out_r = np.empty((nq, kk), dtype=np.int64)
    N.check(lib.rmu_topk_merge(s.ctypes.data, r.ctypes.data, parts, nq, kk, fl, out_s.ctypes.data, out_r.ctypes.data, 0),
            "rmu_topk_merge")
    return out_s, out_r
