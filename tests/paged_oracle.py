"""A NumPy model of the paged key / value cache (semantics at nk_attention_decode_paged_fwd in include/neuronika_hip.h and at
`nn::PageTable` in host/neuronika.hpp): the page table with its reference counts, and gather / scatter between the pools
(num_pages, Hkv, page, dh) and a contiguous (B, Hkv, cap_v, dh) cache.  No test in here: the paged tests import it."""
import numpy as np


class Refused(Exception):
    """what the model raises where `nn::PageTable` panics; the state is untouched"""


class PageTableModel:
    def __init__(self, num_pages, page, max_seqs, max_pages):
        assert page >= 16 and page & (page - 1) == 0
        self.num_pages, self.page, self.max_seqs, self.max_pages = num_pages, page, max_seqs, max_pages
        self.reset()

    def reset(self):
        self.lens = [0] * self.max_seqs
        self.behind = [0] * self.max_seqs
        self.rows = np.full((self.max_seqs, self.max_pages), -1, np.int32)
        self.ref = [0] * self.num_pages
        self.free = set(range(self.num_pages))

    def _seq(self, s):
        if not 0 <= s < self.max_seqs:
            raise Refused("sequence id %d" % s)

    def _unref(self, p):
        self.ref[p] -= 1
        if self.ref[p] == 0:
            self.free.add(p)

    def _take(self):
        p = min(self.free)
        self.free.remove(p)
        self.ref[p] = 1
        return p

    def _pages_of(self, n):
        return (n + self.page - 1) // self.page

    def reserve(self, seqs, T):
        """-> the copies [(old, new)] to make before the append"""
        if T <= 0:
            raise Refused("T")
        left, need, seen = {}, 0, set()
        for s in seqs:
            self._seq(s)
            if s in seen:
                raise Refused("sequence %d twice" % s)
            seen.add(s)
            have, want = self._pages_of(self.lens[s]), self._pages_of(self.lens[s] + T)
            if want > self.max_pages:
                raise Refused("max_pages")
            need += want - have
            if self.lens[s] % self.page:
                last = int(self.rows[s, have - 1])
                if self.ref[last] - left.get(last, 0) > 1:
                    left[last] = left.get(last, 0) + 1
                    need += 1
        if need > len(self.free):
            raise Refused("out of pages")
        copies = []
        for s in seqs:
            have, want = self._pages_of(self.lens[s]), self._pages_of(self.lens[s] + T)
            if self.lens[s] % self.page and self.ref[self.rows[s, have - 1]] > 1:
                old = int(self.rows[s, have - 1])
                self.ref[old] -= 1
                self.rows[s, have - 1] = self._take()
                copies.append((old, int(self.rows[s, have - 1])))
            for i in range(have, want):
                self.rows[s, i] = self._take()
            self.lens[s] += T
        return copies

    def truncate(self, s, n):
        self._seq(s)
        if n < 0 or n > self.lens[s] or n < self.behind[s]:
            raise Refused("truncate")
        for i in range(self._pages_of(n), self._pages_of(self.lens[s])):
            if self.rows[s, i] >= 0:
                self._unref(int(self.rows[s, i]))
                self.rows[s, i] = -1
        self.lens[s] = n

    def release(self, s):
        self._seq(s)
        for i in range(self.max_pages):
            if self.rows[s, i] >= 0:
                self._unref(int(self.rows[s, i]))
                self.rows[s, i] = -1
        self.lens[s] = self.behind[s] = 0

    def fork(self, src, dst):
        self._seq(src)
        self._seq(dst)
        if src == dst or self.lens[dst] != 0 or self.behind[dst] != 0:
            raise Refused("fork")
        self.rows[dst] = self.rows[src]
        for p in self.rows[src]:
            if p >= 0:
                self.ref[p] += 1
        self.lens[dst], self.behind[dst] = self.lens[src], self.behind[src]

    def release_behind(self, s, pos):
        self._seq(s)
        if pos < 0 or pos > self.lens[s]:
            raise Refused("release_behind")
        for i in range(pos // self.page):
            if self.rows[s, i] >= 0:
                self._unref(int(self.rows[s, i]))
                self.rows[s, i] = -1
        self.behind[s] = max(self.behind[s], pos // self.page * self.page)

    def owners(self):
        """how many table entries name each page"""
        cnt = [0] * self.num_pages
        for p in self.rows.ravel():
            if p >= 0:
                cnt[p] += 1
        return cnt


def scatter_rows(Kp, rows, start, table, T, page):
    """the model of nk_kv_pages_append on one pool: Kp (num_pages, H, page, dh) in place, rows (B*T, H*dh), table (B, max_pages)"""
    num_pages, H, _, dh = Kp.shape
    B, max_pages = table.shape
    for b in range(B):
        for t in range(T):
            pos = int(start[b]) + t
            if pos < 0 or pos >= max_pages * page:
                continue
            pg = int(table[b, pos // page])
            if not 0 <= pg < num_pages:
                continue
            Kp[pg, :, pos % page, :] = rows[b * T + t].reshape(H, dh)


def gather_cache(Kp, table, page, fill=0.0):
    """the contiguous (B, H, max_pages * page, dh) cache the table describes; entries outside the pool read as `fill`"""
    num_pages, H, _, dh = Kp.shape
    B, max_pages = table.shape
    out = np.full((B, H, max_pages * page, dh), fill, Kp.dtype)
    for b in range(B):
        for i in range(max_pages):
            pg = int(table[b, i])
            if 0 <= pg < num_pages:
                out[b, :, i * page:(i + 1) * page, :] = Kp[pg]
    return out


def scatter_cache(Kp, cache, table, lens, page):
    """positions [0, lens[b]) of a contiguous (B, H, cap, dh) cache into the pages the table names"""
    for b in range(table.shape[0]):
        for pos in range(int(lens[b])):
            Kp[int(table[b, pos // page]), :, pos % page, :] = cache[b, :, pos, :]
