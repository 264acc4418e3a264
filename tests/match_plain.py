"""A plain NumPy statement of the brute-force matcher's contract.  Test infrastructure only.

Written from the rules of brisk::BruteForceMatcher (brisk/src/brute-force-matcher.cc:80-213) with brisk::Hamming as the
distance, and of cv::DescriptorMatcher's mask helpers - not from the kernels and not from oracle/brisk_oracle_match.c, so
that the two can be held against each other (tests/test_match_plain.py) before either judges a kernel.

  distance   popcount of a ^ b over the first 16 * (dim // 16) bytes
  k-NN       the k smallest of a query's unmasked entries by (distance, image, train index); where fewer exist the
             remaining slots are {trainIdx 0, imgIdx = the last non-empty image, distance 2147483648.0} (the reference
             goes on selecting among entries that all stand at INT_MAX); no non-empty image: no entry at all
  radius     every unmasked entry with float(distance) < max_distance, in the same order
  masked out a query is dropped (no entries) only when EVERY image has a non-empty mask whose row for it is all zero;
             an image without a mask, or without train rows, is not counted and so keeps every query alive

`rows` restricts either function to some queries (the large GPU cases compare a sample); the result is then one array
per listed query, with queryIdx the query's own index.
"""
import numpy as np

DMATCH = np.dtype([("queryIdx", "<i4"), ("trainIdx", "<i4"), ("imgIdx", "<i4"), ("distance", "<f4")])
POP8 = np.array([bin(i).count("1") for i in range(256)], np.uint8)
TOP_UP = np.float32(2147483648.0)


def hamming_row(q, t, table=False):
    """distances of descriptor q to every row of t (n x dim), int64"""
    dim16 = 16 * (t.shape[1] // 16)
    x = np.bitwise_xor(t[:, :dim16], q[None, :dim16])
    if table or not hasattr(np, "bitwise_count"):
        return POP8[x].sum(axis=1, dtype=np.int64)
    return np.bitwise_count(np.ascontiguousarray(x).view(np.uint64)).sum(axis=1, dtype=np.int64)   # the same count, eight bytes at a time


def _sets(query, train, masks):
    query = np.asarray(query, np.uint8)
    train = [np.asarray(t, np.uint8).reshape(-1, query.shape[1]) for t in train]
    start = np.concatenate([[0], np.cumsum([len(t) for t in train])]).astype(np.int64)
    if masks is not None:
        assert len(masks) == len(train)
        masks = [None if m is None else np.asarray(m) for m in masks]
    return query, train, start, masks


def _masked_out(masks, train, q):
    if masks is None or not len(train):
        return False
    for m, t in zip(masks, train):
        if m is None or len(t) == 0 or m[q].any():
            return False
    return True


def _entries(query, train, start, masks, q):
    """(distance, image, train index) of query q's unmasked entries, in image and index order"""
    d, img, idx = [], [], []
    for i, t in enumerate(train):
        if not len(t):
            continue
        di = hamming_row(query[q], t)
        ti = np.arange(len(t), dtype=np.int64)
        if masks is not None and masks[i] is not None:
            keep = masks[i][q] != 0
            di, ti = di[keep], ti[keep]
        d.append(di)
        idx.append(ti)
        img.append(np.full(len(di), i, np.int64))
    if not d:
        z = np.zeros(0, np.int64)
        return z, z, z
    return np.concatenate(d), np.concatenate(img), np.concatenate(idx)


def _records(q, d, img, idx):
    r = np.zeros(len(d), DMATCH)
    r["queryIdx"], r["trainIdx"], r["imgIdx"], r["distance"] = q, idx, img, d.astype(np.float32)
    return r


def match_knn(query, train, k, masks=None, rows=None):
    query, train, start, masks = _sets(query, train, masks)
    nonempty = [i for i, t in enumerate(train) if len(t)]
    out = []
    for q in (range(len(query)) if rows is None else rows):
        q = int(q)
        if _masked_out(masks, train, q) or not nonempty or k <= 0:
            out.append(np.zeros(0, DMATCH))
            continue
        d, img, idx = _entries(query, train, start, masks, q)
        key = (d << 32) | (start[img] + idx)              # (distance, image, train index): images lie in order in `start`
        n = min(k, len(key))
        sel = np.argpartition(key, n - 1)[:n] if 0 < n < len(key) else np.arange(len(key))
        sel = sel[np.argsort(key[sel], kind="stable")]
        r = np.zeros(k, DMATCH)
        r[:n] = _records(q, d[sel], img[sel], idx[sel])
        r[n:]["queryIdx"], r[n:]["trainIdx"], r[n:]["imgIdx"], r[n:]["distance"] = q, 0, nonempty[-1], TOP_UP
        out.append(r)
    return out


def match_radius(query, train, max_distance, masks=None, rows=None):
    query, train, start, masks = _sets(query, train, masks)
    limit = np.float32(max_distance)
    out = []
    for q in (range(len(query)) if rows is None else rows):
        q = int(q)
        if _masked_out(masks, train, q):
            out.append(np.zeros(0, DMATCH))
            continue
        d, img, idx = _entries(query, train, start, masks, q)
        with np.errstate(invalid="ignore"):
            hit = d.astype(np.float32) < limit                # strict; never true for NaN
        d, img, idx = d[hit], img[hit], idx[hit]
        order = np.argsort((d << 32) | (start[img] + idx), kind="stable")
        out.append(_records(q, d[order], img[order], idx[order]))
    return out
