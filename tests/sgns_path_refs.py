"""Device-free side of the SGNS hot-row / fresh-row parity tests (tests/test_sgns_hot_paths_gpu.py, tests/test_n2v_partitioned_gpu.py): WHICH branch of
sgns_win_kernel<.., RELOAD, !ALLC> (gem_amd/csrc/sgns.hpp) every (centre, context) pair of a corpus takes, recomputed on the CPU from the kernel's own
Philox draws (oracle_philox; tags and counter layout of tests/test_oracle_n2v.py::pinned_sgns_on_kernel_draws).  A parity test that runs zero hot rows
passes whatever the hot-row code does; every GPU case therefore asserts floors on these classes before it launches.  tests/test_sgns_path_refs.py ties
the helper to the oracle (same pairs, same targets), so that it cannot drift from what is trained."""
import ctypes as C

import numpy as np

import oracle

INT32_MAX = 2 ** 31 - 1
NEG = 5
FLOOR = 0.05      # every class a case claims to reach holds at least this share of its pairs


def pair_classes(walks, window, seed, epoch, UT, KT, n_slots, key, thr, neg_thr=0, fresh=0, radius=-1, flags=11, walk_id_offset=0, wids=None, bucket=None):
    """The pairs TrainModel forms on `walks` (int32 [nwalks, len]; walk id = wids[i] or walk_id_offset + i), in its order, with the class of each.

    UT / KT / n_slots: the unigram alias table the launch draws from (slot = floor(u n_slots), X = KT[slot] under flags & 2 -- RndUnigramInt's
    quirk -- else the slot, target = X if u' < UT[X] else KT[X]).  bucket = (parts, ctx_part, word_part): a launch of gemhip_sgns_train_part -- only
    pairs with the context in ctx_part and the centre word in word_part, UT / KT the table RESTRICTED to word_part over local rows
    (UT[off[gj]:off[gj + 1]]), targets returned as global ids local * parts + word_part.  key: what the kernel compares with the threshold, indexed by
    GLOBAL node id (the token counts, or the hot key: INT32_MAX for a locally hot node); thr / neg_thr / fresh: SgnsArgs::hot_thr, neg_thr, fresh.
    radius: the cached radius asked for (-1: the default 10), cut at the window as the launch rule does.

    Returns a dict of arrays, one entry per pair:
      ctx, word   the pair (global ids);  targets [np, 5] the negative targets (global ids, including those equal to the centre word)
      special     the pair takes the exact sequential (slow) path, by the rule of stage_fin: a target equals the centre word, a target is drawn twice,
                  or a target occurs in one of the previous two slots (undrawn slots hold target 0, as in the kernel; valid contexts that are not
                  contiguous -- padded walks -- make every pair of the centre special).  bucket launches: the `cross` rule, the previous two slots
                  that have a context of the bucket.
      hot_neg     a target other than the centre word is hot: key >= thr, or under fresh bit 2 key >= neg_thr
      hot_word    the centre word takes the returning-atomic path: key == INT32_MAX, or fresh bit 0 and key >= thr
      hot_ctx     the context never enters the LDS window: key >= thr
      beyond      the context is not hot and no token within `radius` positions of the centre holds its node: fetched per pair, updated by atomic add"""
    walks = np.ascontiguousarray(walks, dtype=np.int32)
    nwalks, length = walks.shape
    L = oracle.lib()
    buf = (C.c_uint32 * 4)()
    UTl = [float(u) for u in np.asarray(UT, dtype=np.float32)]
    KTl = [int(k) for k in KT]
    keyl = [int(k) for k in key]
    parts, gi, gj = bucket if bucket is not None else (1, 0, 0)
    quirk = (flags & 2) != 0
    R = min(10 if radius < 0 else radius, window, 31)
    out = {k: [] for k in ('ctx', 'word', 'targets', 'special', 'hot_neg', 'hot_word', 'hot_ctx', 'beyond')}

    def philox(c0, c1, c2, c3):
        L.oracle_philox(C.c_uint64(seed), C.c_uint32(c0), C.c_uint32(c1), C.c_uint32(c2), C.c_uint32(c3), buf)
        return buf[0], buf[1]

    for wl in range(nwalks):
        walk = [int(v) for v in walks[wl]]
        wid = int(wids[wl]) if wids is not None else walk_id_offset + wl
        w_lo, w_hi = wid & 0xFFFFFFFF, (wid >> 32) & 0xFFFFFFFF
        for pos in range(length):
            word = walk[pos]
            if word < 0 or word % parts != gj:
                continue
            b = philox(w_lo, w_hi, pos, 2 | (epoch << 8))[0] % window            # TAG_WIN
            tg = [[0] * NEG for _ in range(2 * window)]                           # by slot ai (the window without its centre); undrawn: target 0
            valid = []
            for a in range(b, 2 * window + 1 - b):
                cp = pos - window + a
                if a == window or cp < 0 or cp >= length:
                    continue
                ai = a if a < window else a - 1
                for j in range(1, NEG + 1):
                    x, y = philox(w_lo, w_hi, pos | (a << 16), 3 | (epoch << 8) | (j << 16))      # TAG_NEG
                    slot = (x * n_slots) >> 32
                    X = KTl[slot] if quirk else slot
                    loc = X if (y >> 8) / 16777216.0 < UTl[X] else KTl[X]
                    tg[ai][j - 1] = loc * parts + gj
                if walk[cp] >= 0 and walk[cp] % parts == gi:
                    valid.append((ai, cp))
            contiguous = all(valid[k + 1][0] == valid[k][0] + 1 for k in range(len(valid) - 1))
            for k, (ai, cp) in enumerate(valid):
                t = tg[ai]
                sp = word in t or len(set(t)) < NEG
                if bucket is None:
                    prev = [tg[q] for q in (ai - 1, ai - 2) if q >= 0]
                    sp = sp or not contiguous
                else:
                    prev = [tg[valid[q][0]] for q in (k - 1, k - 2) if q >= 0]
                sp = sp or any(u in t for p in prev for u in p)
                ctx = walk[cp]
                hot_neg = any(u != word and (keyl[u] >= thr or ((fresh & 4) and keyl[u] >= neg_thr)) for u in t)
                hot_ctx = keyl[ctx] >= thr
                out['ctx'].append(ctx); out['word'].append(word); out['targets'].append(t)
                out['special'].append(sp); out['hot_neg'].append(hot_neg); out['hot_ctx'].append(hot_ctx)
                out['hot_word'].append(keyl[word] == INT32_MAX or bool((fresh & 1) and keyl[word] >= thr))
                out['beyond'].append(not hot_ctx and ctx not in walk[max(0, pos - R):pos + R + 1])
    res = {k: np.asarray(out[k], dtype=bool) for k in ('special', 'hot_neg', 'hot_word', 'hot_ctx', 'beyond')}
    res['ctx'] = np.asarray(out['ctx'], dtype=np.int32); res['word'] = np.asarray(out['word'], dtype=np.int32)
    res['targets'] = np.asarray(out['targets'], dtype=np.int32).reshape(-1, NEG)
    return res


def shares(cls):
    """Fraction of the pairs in each class the GPU cases put floors on."""
    n = float(max(1, len(cls['ctx'])))
    sp, hn = cls['special'], cls['hot_neg']
    return {'pairs': len(cls['ctx']), 'fast_hot': (~sp & hn).sum() / n, 'fast_cold': (~sp & ~hn).sum() / n, 'slow': sp.sum() / n,
            'slow_hot': (sp & hn).sum() / n, 'hot_word': cls['hot_word'].sum() / n, 'hot_ctx': cls['hot_ctx'].sum() / n, 'beyond': cls['beyond'].sum() / n}


def assert_floors(cls, names, floor=FLOOR):
    """Every class in `names` holds at least `floor` of the pairs; returns the shares (the caller prints them)."""
    s = shares(cls)
    assert s['pairs'] > 100, s
    for k in names:
        assert s[k] >= floor, (k, s)
    return s


def updated_neg_rows(cls):
    """The SynNeg rows TrainModel touches on these pairs: every centre word, every target that is not its pair's centre word."""
    rows = set(cls['word'].tolist())
    keep = cls['targets'] != cls['word'][:, None]
    rows.update(cls['targets'][keep].tolist())
    return rows
