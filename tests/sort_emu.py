"""A numpy / plain-Python emulation of the sort-based analysis kernels of csrc/bnr_analysis_kernels.h, in the kernels' own order of work, with
switchable defects: what tests/test_sort_edges_host.py uses to show that the rows of tests/sort_cases.py tell a subtly wrong kernel from a
right one.  It is not a reference -- the references are np.sort, scipy's rankdata and incl_ref.brute -- but a model of the kernels' structure:

  bnr_sort_build_keys   the key image, the eight digit histograms, a pass is skipped where one digit holds all n keys
  bnr_sort_passes       per live pass the exclusive scan of the digit counts (base), then tiles of 256 keys in order; in a tile every wave of 64
                        counts its keys per digit (wcnt), a key goes to base[d] + its rank among the wave's keys of digit d + the counts of the
                        lower waves, and base[d] then advances by every wave's count; the two buffers change roles after a live pass only
  k_rank phase 3, 4     per tile the heads' ballot per wave, the last head of each wave (wlast), the carry into the next tile; sa, ea; the ranks
  k_hdi phase 3, 4      the two binary searches over the sorted keys; per level the strided scan of the 256 threads and the tree over them
  k_incl_group          the gather and sort per pattern word, the run heads, the sort of the counts

DEFECTS names the deliberate mistakes; `defect=None` is the kernels as written."""
import numpy as np

import sort_cases as sc

U = np.uint64
NT, WAVE = 256, 64
STALE = 0xDEADBEEF                                                      # what an entry of sa / ea holds that no thread wrote
DEFECTS = {
    1: "the buffers also change roles at a skipped pass that lies between two live ones",
    2: "the running base advances once per tile: a wave does not add the counts of the waves below it (an unstable scatter)",
    3: "the carry is lost in a tile that holds no head",
    4: "the ea write of the final run is dropped when t = n - 1 is itself a head",
    5: "the HDI tie is broken by thread and not by j",
    6: "both sign searches use <",
}


# ------------------------------------------------------------------------------------------------------------------ the sort
def histograms(keys):
    return np.stack([np.bincount(((keys >> U(8 * b)) & U(255)).astype(np.int64), minlength=256) for b in range(8)])


def sort_passes(keys, idx=None, defect=None):
    """bnr_sort_passes<IDX>: (sorted keys, their indices or None, the free key buffer, the number of live passes)"""
    n = keys.size
    hist = histograms(keys)
    skip = [bool((hist[b] == n).any()) for b in range(8)]
    src, dst = keys.copy(), np.zeros(n, dtype=U)
    si, di = (idx.copy(), np.zeros(n, dtype=np.int64)) if idx is not None else (None, None)
    live = [b for b in range(8) if not skip[b]]
    for p in range(8):
        if skip[p]:
            if defect == 1 and live and live[0] < p < live[-1]:
                src, dst, si, di = dst, src, di, si
            continue
        base = np.cumsum(hist[p]) - hist[p]
        for t0 in range(0, n, NT):
            tile = src[t0:t0 + NT]
            d = ((tile >> U(8 * p)) & U(255)).astype(np.int64)
            pos = np.empty(tile.size, dtype=np.int64)
            below = np.zeros(256, dtype=np.int64)                       # the counts of the lower waves of this tile
            for w0 in range(0, tile.size, WAVE):
                dw = d[w0:w0 + WAVE]
                order = np.argsort(dw, kind="stable")
                ds = dw[order]
                start = np.flatnonzero(np.append(True, ds[1:] != ds[:-1]))
                lrank = np.empty(dw.size, dtype=np.int64)
                lrank[order] = np.arange(dw.size) - np.repeat(start, np.diff(np.append(start, dw.size)))
                pos[w0:w0 + WAVE] = base[dw] + lrank + (0 if defect == 2 else below[dw])
                below += np.bincount(dw, minlength=256)
            base = base + below
            ok = pos < n
            dst[pos[ok]] = tile[ok]
            if si is not None:
                di[pos[ok]] = si[t0:t0 + NT][ok]
        src, dst, si, di = dst, src, di, si
    return src, si, dst, len(live)


# ------------------------------------------------------------------------------------------------------------------ k_rank
def rank_row(x, defect=None):
    """k_rank's ranks of a NaN-free row (all = 1, one window)"""
    x = np.asarray(x, dtype=np.float64)
    n = x.size
    src, si, _free, _ = sort_passes(sc.key_of(x), np.arange(n, dtype=np.int64), defect)
    sa = np.full(n, STALE, dtype=np.int64)
    ea = np.full(n, STALE, dtype=np.int64)
    carry = 0
    for t0 in range(0, n, NT):
        t = np.arange(t0, min(t0 + NT, n))
        head = np.ones(t.size, dtype=bool)
        prev = src[np.maximum(t - 1, 0)]
        head[t > 0] = (src[t] != prev)[t > 0]
        c = carry                                                       # the last head of the lower waves, or the carry
        s_in = np.empty(t.size, dtype=np.int64)
        sx = np.empty(t.size, dtype=np.int64)
        for w0 in range(0, t.size, WAVE):
            hw, tw = head[w0:w0 + WAVE], t[w0:w0 + WAVE]
            last_in = np.maximum.accumulate(np.where(hw, tw, -1))       # the last head at or below the lane
            last_lo = np.append(-1, last_in[:-1])                       # ... strictly below it
            s_in[w0:w0 + WAVE] = np.where(last_in >= 0, last_in, c)
            sx[w0:w0 + WAVE] = np.where(last_lo >= 0, last_lo, c)
            if hw.any():
                c = int(tw[hw][-1])
        sa[t] = s_in
        hs = head & (t > 0)
        ea[sx[hs]] = t[hs]
        if t[-1] == n - 1 and not (defect == 4 and head[-1]):
            ea[s_in[-1]] = n
        if t.size == NT:                                                # (thread 255 holds a key)
            carry = int(s_in[-1])
            if defect == 3 and not head.any():
                carry = 0
    r = np.full(n, -1.0)
    r[si] = (sa + ea[np.minimum(sa, n - 1)] + 1) * 0.5
    return r


# ------------------------------------------------------------------------------------------------------------------ k_hdi
ZERO = U(1) << U(63)


def _search(src, strict):
    """the first position whose key is >= (strict) or > the key of +0"""
    lo, hi = 0, src.size
    while lo < hi:
        mid = lo + (hi - lo) // 2
        k = src[mid]
        if (k < ZERO) if strict else (k <= ZERO):
            lo = mid + 1
        else:
            hi = mid
    return lo


def hdi_row(x, ws, defect=None):
    """k_hdi of a finite row for the window lengths `ws`: (lower, upper per w, median, p_pos, p_neg)"""
    x = np.asarray(x, dtype=np.float64)
    n = x.size
    src = sort_passes(sc.key_of(x), None, defect)[0]
    xs = sc.double_of(src)
    p_neg = _search(src, True) / float(n)
    p_pos = (n - _search(src, defect == 6)) / float(n)
    with np.errstate(over="ignore", invalid="ignore"):
        med = (xs[n // 2 - 1] + xs[n // 2]) / 2.0 if n >= 2 else xs[0]
    lower, upper = [], []
    for w in ws:
        m = n - w
        rd, rj = np.full(NT, np.inf), np.full(NT, 0x7FFFFFFF, dtype=np.int64)
        with np.errstate(over="ignore", invalid="ignore"):
            d = xs[w:] - xs[:m]
        for tid in range(min(NT, m)):
            mine = d[tid::NT]
            k = int(np.argmin(mine))                                    # the first smallest of the thread's own windows
            rd[tid], rj[tid] = mine[k], tid + NT * k
        tie = np.arange(NT) if defect == 5 else rj                      # what breaks a tie of the widths: j, or the thread that holds it
        s = NT // 2
        while s > 0:
            a, b = slice(0, s), slice(s, 2 * s)
            take = (rd[b] < rd[a]) | ((rd[b] == rd[a]) & (tie[b] < tie[a]))
            rd[a], rj[a], tie[a] = np.where(take, rd[b], rd[a]), np.where(take, rj[b], rj[a]), np.where(take, tie[b], tie[a])
            s //= 2
        j = int(rj[0])
        lower.append(xs[j])
        upper.append(xs[j + w])
    return np.array(lower), np.array(upper), med, p_pos, p_neg


# ------------------------------------------------------------------------------------------------------------------ k_incl_group
def incl_group(words, ntop, defect=None):
    """k_incl_group of S x W pattern words: (n_distinct, top_sets (ntop, W), top_count (ntop,))"""
    words = np.ascontiguousarray(words, dtype=U)
    S, W = words.shape
    si = np.arange(S, dtype=np.int64)
    for wd in range(W):
        _keys, si, _free, _ = sort_passes(words[si, wd], si, defect)
    sw = words[si]
    head = np.append(True, (sw[1:] != sw[:-1]).any(axis=1))
    at = np.flatnonzero(head)
    nd = at.size
    cnt = np.diff(np.append(at, S))
    keys = ((U(0xFFFFFFFF) - cnt.astype(U)) << U(32)) | at.astype(U)
    keys = sort_passes(keys, None, defect)[0]
    top_sets, top_count = np.zeros((ntop, W), dtype=U), np.zeros(ntop, dtype=np.int64)
    k = min(ntop, nd)
    top_count[:k] = (U(0xFFFFFFFF) - (keys[:k] >> U(32))).astype(np.int64)
    top_sets[:k] = words[si[np.minimum((keys[:k] & U(0xFFFFFFFF)).astype(np.int64), S - 1)]]
    return nd, top_sets, top_count
