"""CPU references of the SSD losses and their gradients (ron_ssd_losses / ron_ssd_losses_grad; no GPU, no TensorFlow).

Every function takes the flat inputs of one batch: ``x`` [rows, C] float32 logits, ``loc`` / ``gloc`` [rows, 4], ``g`` [rows] int64
classes, ``s`` [rows] float32 scores, the rows in the order (layer, image, row, column, anchor); ``layer_rows`` the row count of every
layer, ``N`` the batch size, ``mining`` 'batch' or 'layer'.

  * ``mine``            the selection itself on any array of values: counts [S, 4], the mined mask, t per segment.  Used on float64
                        values by the reference, on float32 ones by the emulation, and by the GPU tests on the device's own values.
  * ``losses_ref``      float64, analytic: losses, counts, masks, gradients and the per-row terms the bound needs.
  * ``losses_torch``    the second, independent reference: torch-CPU float64 (softmax, topk, cross_entropy, autograd).
  * ``losses_emulated`` float32 emulation of the kernels' arithmetic, with the mutants of ``MUTANTS`` as switches.
  * ``losses_bound``, ``grad_bound``, ``p0_bound``  bounds of |kernel - float64 reference|: the error model
                        of encode_ref.losses_bound / loss_grad_ref.grad_bound extended by abs_smooth.
"""
import numpy as np

import encode_ref as er
import loss_grad_ref as gr

F = np.float32
U = 2.0 ** -24
EXP_ULP = gr.EXP_ULP
TINY = 2.0 ** -126
MUTANTS = ('le_threshold', 'mine_k_by_index', 'kth_among_candidates', 'no_plus_n', 'round_k', 'batch_per_layer', 'layer_over_batch',
           'loc_div_n_pos', 'ge_match', 'ignored_as_candidates', 'mined_label_g')
COUNTS = ('n_pos', 'n_cand', 'k', 'n_mined')


def segments(layer_rows, mining):
    """[(first row, one past the last)] per segment: the whole batch, or one per layer."""
    edges = np.concatenate([[0], np.cumsum(layer_rows)]).astype(np.int64)
    if mining == 'batch':
        return [(0, int(edges[-1]))]
    assert mining == 'layer'
    return [(int(edges[i]), int(edges[i + 1])) for i in range(len(layer_rows))]


def row_sets(s, match_threshold=0.5, mut=()):
    s = np.asarray(s, F)
    pos = (s >= F(match_threshold)) if 'ge_match' in mut else (s > F(match_threshold))
    cand = ~pos & ((s > F(-np.inf)) if 'ignored_as_candidates' in mut else (s > F(-0.5)))
    return pos, cand


def segment_k(n_pos, n_cand, R, N, negative_ratio, mining, mut=()):
    f = F(negative_ratio) * F(n_pos)                            # a float32 product
    want = int(np.round(f)) if 'round_k' in mut else int(f)     # tf.cast truncates
    if mining == 'batch':
        k = min(want + (0 if 'no_plus_n' in mut else N), n_cand)
    else:
        k = min(max(want, R // 8, 4 * N), 1 + n_cand)
    return max(min(k, R), 0)


def mine(v, pos, cand, layer_rows, N, mining, negative_ratio=3., mut=()):
    """The hard-negative selection on the values v ([rows], candidates' p0, 1 elsewhere).  Returns (counts int32 [S, 4], mined bool
    [rows], t per segment (None where k == 0))."""
    if 'batch_per_layer' in mut and mining == 'batch':
        segs = segments(layer_rows, 'layer')
    elif 'layer_over_batch' in mut and mining == 'layer':
        segs = segments(layer_rows, 'batch')
    else:
        segs = segments(layer_rows, mining)
    v = np.asarray(v)
    mined = np.zeros(v.shape[0], bool)
    counts, ts = [], []
    for lo, hi in segs:
        vv, cc = v[lo:hi], cand[lo:hi]
        n_pos, n_cand, R = int(pos[lo:hi].sum()), int(cc.sum()), hi - lo
        k = segment_k(n_pos, n_cand, R, N, negative_ratio, mining, mut)
        t = None
        if k > 0:
            if 'kth_among_candidates' in mut:
                pool = np.sort(vv[cc])
                t = pool[min(k, pool.size) - 1] if pool.size else vv.dtype.type(1)
            else:
                t = np.sort(vv)[k - 1]
            if 'mine_k_by_index' in mut:
                m = np.zeros(R, bool)
                m[np.argsort(vv, kind='stable')[:k]] = True
                m &= cc
            elif 'le_threshold' in mut:
                m = cc & (vv <= t)
            else:
                m = cc & (vv < t)
            mined[lo:hi] = m
        counts.append([n_pos, n_cand, k, int(mined[lo:hi].sum())])
        ts.append(t)
    return np.array(counts, np.int32), mined, ts


def softmax64(x32):
    x = np.asarray(x32, F).astype(np.float64)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def abs_smooth(d):
    a = np.abs(d)
    return 0.5 * ((a - 1) * np.minimum(a, 1) + a)


def _labels(g, C):
    return np.clip(np.asarray(g).reshape(-1), 0, C).astype(np.int64)


def _lse_rows(x64, label):
    """Cross-entropy rows in float64; NaN where the label is out of range."""
    C = x64.shape[1]
    out = np.full(x64.shape[0], np.nan)
    ok = label < C
    if ok.any():
        out[ok] = er._lse_rows(x64[ok], label[ok])
    return out


def _term_scales(counts, N, alpha, mining, dtype=np.float64):
    """Per segment (s_pos, s_neg, s_loc): the divisors of the three terms, 0 where the term is 0."""
    out = []
    a = dtype(F(alpha))
    for n_pos, _, _, n_mined in counts:
        if mining == 'batch':
            out.append((dtype(1) / dtype(N), dtype(1) / dtype(N), a / dtype(N)))
        else:
            out.append((dtype(1) / dtype(n_pos) if n_pos > 0 else dtype(0), dtype(1) / dtype(n_mined) if n_mined > 0 else dtype(0),
                        a / dtype(4 * n_pos) if (n_pos > 0 and a != 0) else dtype(0)))
    return out


def losses_ref(x, loc, g, gloc, s, layer_rows, N, mining, match_threshold=0.5, negative_ratio=3., alpha=1., mined=None):
    """float64 reference.  `mined`, when given, replaces the reference's own selection (the GPU tests hand over the mask that the
    device's own values give).  Returns a dict: losses [4], counts [S, 4], pos / cand / mined, v (float64), d_cls, d_loc, and the
    per-row terms."""
    x, loc, gloc = np.asarray(x, F), np.asarray(loc, F), np.asarray(gloc, F)
    rows, C = x.shape
    pos, cand = row_sets(s, match_threshold)
    p = softmax64(x)
    v = np.where(cand, p[:, 0], 1.0)
    counts, own, ts = mine(v, pos, cand, layer_rows, N, mining, negative_ratio)
    segs = segments(layer_rows, mining)
    if mined is None:
        mined = own
    else:
        mined = np.asarray(mined, bool)
        counts = counts.copy()
        counts[:, 3] = [int(mined[lo:hi].sum()) for lo, hi in segs]
    lab = _labels(g, C)
    x64 = x.astype(np.float64)
    ce_pos = np.zeros(rows)
    ce_pos[pos] = _lse_rows(x64[pos], lab[pos])
    ce_neg = np.zeros(rows)
    ce_neg[mined] = _lse_rows(x64[mined], np.zeros(int(mined.sum()), np.int64))
    d64 = loc.astype(np.float64) - gloc.astype(np.float64)
    sl = np.zeros(rows)
    sl[pos] = abs_smooth(d64[pos]).sum(axis=1)
    scales = _term_scales(counts, N, alpha, mining)
    terms = np.zeros((len(segs), 3))
    d_cls, d_loc = np.zeros((rows, C)), np.zeros((rows, 4))
    onehot = lambda l: (np.arange(C)[None, :] == l[:, None]).astype(np.float64)
    for i, (lo, hi) in enumerate(segs):
        sp, sn, sloc = scales[i]
        sel = slice(lo, hi)
        terms[i] = [ce_pos[sel].sum() * sp if sp else 0.0, ce_neg[sel].sum() * sn if sn else 0.0, sl[sel].sum() * sloc if sloc else 0.0]
        pp, mm = pos[sel], mined[sel]
        blk = d_cls[sel]
        blk[pp] = (p[sel][pp] - onehot(lab[sel][pp])) * sp
        blk[pp & (lab[sel] >= C)] = np.nan
        blk[mm] = (p[sel][mm] - onehot(np.zeros(int(mm.sum()), np.int64))) * sn
        dl = d_loc[sel]
        dl[pp] = np.clip(d64[sel][pp], -1.0, 1.0) * sloc
    tot = terms.sum(axis=0)
    losses = np.array([tot[0], tot[1], tot[2], tot[0] + tot[1] + tot[2]])
    return dict(losses=losses, counts=counts, pos=pos, cand=cand, mined=mined, v=v, t=ts, d_cls=d_cls, d_loc=d_loc, softmax=p, labels=lab,
                ce_pos=ce_pos, ce_neg=ce_neg, sl=sl, terms=terms, scales=scales, segs=segs)


# ------------------------------------------------------------------------------------------------------------ torch, independent
def losses_torch(x, loc, g, gloc, s, layer_rows, N, mining, match_threshold=0.5, negative_ratio=3., alpha=1.):
    """What a user would compose from torch on the CPU, in float64: softmax, topk of the negated values, cross_entropy, autograd.
    Rows whose label is out of range are left out of the sum (torch refuses them); their gradient rows are returned as NaN and
    the class term as NaN."""
    import torch
    import torch.nn.functional as TF
    xt = torch.from_numpy(np.asarray(x, F).astype(np.float64)).requires_grad_(True)
    lt = torch.from_numpy(np.asarray(loc, F).astype(np.float64)).requires_grad_(True)
    gt = torch.from_numpy(np.asarray(gloc, F).astype(np.float64))
    st = torch.from_numpy(np.asarray(s, F))
    C = xt.shape[1]
    lab = torch.from_numpy(_labels(g, C))
    a = float(F(alpha))
    total = [torch.zeros((), dtype=torch.float64) for _ in range(3)]
    counts, mined_all, bad = [], torch.zeros(xt.shape[0], dtype=torch.bool), False
    for lo, hi in segments(layer_rows, mining):
        xs, sc = xt[lo:hi], st[lo:hi]
        pmask = sc > float(F(match_threshold))
        nmask = ~pmask & (sc > -0.5)
        n_pos, n_cand, R = int(pmask.sum()), int(nmask.sum()), hi - lo
        p0 = torch.softmax(xs.detach(), dim=1)[:, 0]
        nvalues = torch.where(nmask, p0, torch.ones_like(p0))
        want = int(float(F(negative_ratio) * F(n_pos)))
        k = min(want + N, n_cand) if mining == 'batch' else min(max(want, R // 8, 4 * N), 1 + n_cand)
        k = max(min(k, R), 0)
        mined = torch.zeros(R, dtype=torch.bool)
        if k > 0:
            val, _ = torch.topk(-nvalues, k)
            mined = nmask & (nvalues < -val[-1])
        mined_all[lo:hi] = mined
        n_mined = int(mined.sum())
        counts.append([n_pos, n_cand, k, n_mined])
        ok = pmask & (lab[lo:hi] < C)
        bad = bad or bool((pmask & ~ok).any())
        ce_p = TF.cross_entropy(xs[ok], lab[lo:hi][ok], reduction='sum') if ok.any() else torch.zeros((), dtype=torch.float64)
        ce_n = TF.cross_entropy(xs[mined], torch.zeros(n_mined, dtype=torch.int64), reduction='sum') if n_mined else torch.zeros((), dtype=torch.float64)
        d = (lt[lo:hi] - gt[lo:hi])[pmask]
        absx = d.abs()
        sl = (0.5 * ((absx - 1) * torch.clamp(absx, max=1.0) + absx)).sum()
        if mining == 'batch':
            total[0] = total[0] + ce_p / N
            total[1] = total[1] + ce_n / N
            total[2] = total[2] + a * sl / N
        else:
            if n_pos > 0:
                total[0] = total[0] + ce_p / n_pos
            if n_mined > 0:
                total[1] = total[1] + ce_n / n_mined
            if n_pos > 0 and a != 0:
                total[2] = total[2] + a * sl / (4 * n_pos)
    tot = total[0] + total[1] + total[2]
    if tot.requires_grad:
        tot.backward()
    d_cls = xt.grad.numpy() if xt.grad is not None else np.zeros(tuple(xt.shape))
    d_loc = lt.grad.numpy() if lt.grad is not None else np.zeros(tuple(lt.shape))
    pos_all, _ = row_sets(s, match_threshold)
    d_cls[pos_all & (lab.numpy() >= C)] = np.nan
    losses = np.array([float(t.detach()) for t in total] + [float(tot.detach())])
    if bad:
        losses[[0, 3]] = np.nan
    return dict(losses=losses, counts=np.array(counts, np.int32), mined=mined_all.numpy(), d_cls=d_cls, d_loc=d_loc)


# ------------------------------------------------------------------------------------------------------------ float32 emulation
def _softmax32(x):
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        mx = x.max(axis=1)
        e = np.exp(x - mx[:, None])
        tot = np.zeros(x.shape[0], F)
        for i in range(x.shape[1]):                            # in index order, as the kernels add them
            tot = tot + e[:, i]
        p = e / tot[:, None]
    assert p.dtype == F
    return p, mx, tot


def _ce32(x, mx, tot, label):
    C = x.shape[1]
    with np.errstate(invalid='ignore', divide='ignore'):
        v = (np.log(tot) + mx) - x[np.arange(x.shape[0]), np.minimum(label, C - 1)]
    v = v.astype(F)
    v[label >= C] = np.nan
    return v


def abs_smooth32(d):
    a = np.abs(d)
    r = F(0.5) * ((a - F(1)) * np.minimum(a, F(1)) + a)
    assert r.dtype == F
    return r


def losses_emulated(x, loc, g, gloc, s, layer_rows, N, mining, match_threshold=0.5, negative_ratio=3., alpha=1., mut=()):
    """float32 rows, float64 accumulation, float32 divisions: the kernels' arithmetic (numpy's expf / logf in place of the
    device's).  Returns losses float32 [4], counts, pos / cand / mined, v float32, d_cls, d_loc."""
    x, loc, gloc = np.asarray(x, F), np.asarray(loc, F), np.asarray(gloc, F)
    rows, C = x.shape
    pos, cand = row_sets(s, match_threshold, mut)
    p, mx, tot = _softmax32(x)
    v = np.where(cand, p[:, 0], F(1))
    counts, mined, ts = mine(v, pos, cand, layer_rows, N, mining, negative_ratio, mut)
    segs = segments(layer_rows, mining)
    if len(counts) != len(segs):                               # a mutant that mined over other segments: recount per real segment
        counts = np.array([[int(pos[lo:hi].sum()), int(cand[lo:hi].sum()), -1, int(mined[lo:hi].sum())] for lo, hi in segs], np.int32)
    lab = _labels(g, C)
    neg_lab = lab if 'mined_label_g' in mut else np.zeros(rows, np.int64)
    ce_pos = np.where(pos, _ce32(x, mx, tot, lab), F(0)).astype(np.float64)
    ce_neg = np.where(mined, _ce32(x, mx, tot, neg_lab), F(0)).astype(np.float64)
    d = loc - gloc
    sm = abs_smooth32(d)
    sl = np.where(pos, ((sm[:, 0] + sm[:, 1]) + sm[:, 2]) + sm[:, 3], F(0)).astype(np.float64)
    a = F(alpha)
    quad = 1 if 'loc_div_n_pos' in mut else 4
    out = np.zeros(3, F)
    d_cls, d_loc = np.zeros((rows, C), F), np.zeros((rows, 4), F)
    onehot = lambda l: (np.arange(C)[None, :] == l[:, None]).astype(F)
    for i, (lo, hi) in enumerate(segs):
        n_pos, n_mined = int(counts[i][0]), int(counts[i][3])
        sums = [F(ce_pos[lo:hi].sum()), F(ce_neg[lo:hi].sum()), F(sl[lo:hi].sum())]
        with np.errstate(invalid='ignore'):
            if mining == 'batch':
                t3 = [sums[0] / F(N), sums[1] / F(N), a * (sums[2] / F(N))]
                sc = (F(1) / F(N), F(1) / F(N), a / F(N))
            else:
                okl = n_pos > 0 and a != 0
                t3 = [sums[0] / F(n_pos) if n_pos > 0 else F(0), sums[1] / F(n_mined) if n_mined > 0 else F(0),
                      a * (sums[2] / F(quad * n_pos)) if okl else F(0)]
                sc = (F(1) / F(n_pos) if n_pos > 0 else F(0), F(1) / F(n_mined) if n_mined > 0 else F(0),
                      a / F(quad * n_pos) if okl else F(0))
            out = np.array(t3, F) if i == 0 else (out + np.array(t3, F)).astype(F)
            sel = slice(lo, hi)
            pp, mm = pos[sel], mined[sel]
            blk = d_cls[sel]
            blk[pp] = (p[sel][pp] - onehot(lab[sel][pp])) * sc[0]
            blk[pp & (lab[sel] >= C)] = np.nan
            blk[mm] = (p[sel][mm] - onehot(neg_lab[sel][mm])) * sc[1]
            d_loc[sel][pp] = np.clip(d[sel][pp], F(-1), F(1)) * sc[2]
    with np.errstate(invalid='ignore'):
        losses = np.array([out[0], out[1], out[2], (out[0] + out[1]) + out[2]], F)
    return dict(losses=losses, counts=counts, pos=pos, cand=cand, mined=mined, v=v, d_cls=d_cls, d_loc=d_loc)


# ------------------------------------------------------------------------------------------------------------ the bounds
def p0_bound(x32):
    """|device p0 - float64 p0| per row: the softmax element of loss_grad_ref._rows_bound (u |z_k| on the argument, EXP_ULP ulp of
    expf, C - 1 ordered additions, one correctly rounded division), for k = 0."""
    x = np.asarray(x32, F).astype(np.float64)
    C = x.shape[1]
    z = x - x.max(axis=1, keepdims=True)
    e = np.exp(z)
    S = e.sum(axis=1, keepdims=True)
    a = U * np.abs(z) + 2 * EXP_ULP * U
    r = (e * a).sum(axis=1, keepdims=True) / S + (C - 1) * U
    p = e / S
    return ((p * (a + r + U) + TINY / S + TINY) * 1.0001)[:, 0]


def _ce_rows_bound(x32, label):
    """encode_ref.losses_bound's cross-entropy row (its derivation is in that docstring), for rows with a label in range."""
    x = np.asarray(x32, F).astype(np.float64)
    C = x.shape[1]
    mx = x.max(axis=1)
    z = x - mx[:, None]
    e = np.exp(z)
    ssum = e.sum(axis=1)
    rel_s = (e * (U * np.abs(z) + EXP_ULP * 2 * U)).sum(axis=1) / ssum + (C - 1) * U
    L = np.log(ssum)
    logf_err = er.LOGF_ULP * np.spacing(np.abs(L).astype(F)).astype(np.float64)
    tail = 2 * U * (np.abs(L) + np.abs(mx) + np.abs(x[np.arange(x.shape[0]), np.minimum(label, C - 1)]))
    return (rel_s * 1.0001 + logf_err + tail) * (1 + 1e-6)


def _abs_smooth_rows_bound(loc, gloc):
    """One abs_smooth row, r = 0.5 ((a - 1) min(a, 1) + a) with a = |fl(p - t)|, summed over four coordinates in float32:
        d = fl(p - t)     u |d|; r is 1-Lipschitz in a (r' = a below 1, 1 above), so this moves r by at most u a
        a - 1             one rounding: u |a - 1|, carried through the product with m = min(a, 1) <= 1: u |a - 1| m
        (a - 1) m         one rounding: u |(a - 1) m|
        ... + a           one rounding: u |(a - 1) m + a|
        0.5 *             exact
    so 0.5 (2 u |a - 1| m + u |(a - 1) m + a|) + u a per coordinate, and 3 u of the row's sum for its three float32 additions."""
    d = np.abs(np.asarray(loc, F).astype(np.float64) - np.asarray(gloc, F).astype(np.float64))
    m = np.minimum(d, 1.0)
    per = 0.5 * (2 * U * np.abs(d - 1) * m + U * np.abs((d - 1) * m + d)) + U * d
    return (per.sum(axis=1) + 3 * U * abs_smooth(d).sum(axis=1)) * (1 + 1e-6)


def losses_bound(x, loc, gloc, ref, alpha=1.):
    """Bound of |kernel - float64 reference| for the four losses, for a result of losses_ref.  Rows: the two bounds above.  The
    rows are added in float64 (2^-40 relative covers it); a term is one rounding of the sum to float32, one division and, for the
    localisation, one product with alpha: 4 u relative.  LAYER adds the layers in float32 (S - 1 additions on the running sum), the
    total two more: u times the sum of the terms' magnitudes each."""
    x = np.asarray(x, F)
    pos, mined = ref['pos'], ref['mined']
    rows = x.shape[0]
    b_pos, b_neg, b_loc = np.zeros(rows), np.zeros(rows), np.zeros(rows)
    ok = pos & (ref['labels'] < x.shape[1])
    if ok.any():
        b_pos[ok] = _ce_rows_bound(x[ok], ref['labels'][ok])
    if mined.any():
        b_neg[mined] = _ce_rows_bound(x[mined], np.zeros(int(mined.sum()), np.int64))
    if pos.any():
        b_loc[pos] = _abs_smooth_rows_bound(np.asarray(loc, F)[pos], np.asarray(gloc, F)[pos])
    rel = 2.0 ** -40 + 4 * U * (1 + 1e-6)
    out = np.zeros(3)
    mag = np.zeros(3)
    S = len(ref['segs'])
    for i, (lo, hi) in enumerate(ref['segs']):
        sc = [abs(float(v)) for v in ref['scales'][i]]
        vals = (np.nansum(np.abs(ref['ce_pos'][lo:hi])), np.abs(ref['ce_neg'][lo:hi]).sum(), np.abs(ref['sl'][lo:hi]).sum())
        for k, b in enumerate((b_pos, b_neg, b_loc)):
            out[k] += sc[k] * (b[lo:hi].sum() + rel * vals[k]) + TINY
            mag[k] += sc[k] * vals[k]
    out += (S - 1) * U * mag * (1 + 1e-6)
    total = out.sum() + 2 * U * mag.sum() * (1 + 1e-6)
    return np.append(out, total)


def grad_bound(x, loc, gloc, ref):
    """(bound_cls [rows, C], bound_loc [rows, 4]) for a result of losses_ref; 0 outside the sets (those elements are exactly 0).  The
    class rows are loss_grad_ref._rows_bound with the row's own scale.  A localisation element is clamp(fl(p - t), -1, 1) * s: the
    clamp is continuous, so u |d| from the subtraction where |d| < 1 (nothing beyond: +-1 is exact), s = fl(alpha / n) carries u
    and the product one more: |s| u |d| + 2 u |clamp(d) s|, plus 2^-126 where the product is subnormal."""
    x = np.asarray(x, F)
    rows, C = x.shape
    b_cls, b_loc = np.zeros((rows, C)), np.zeros((rows, 4))
    d = np.abs(np.asarray(loc, F).astype(np.float64) - np.asarray(gloc, F).astype(np.float64))
    for i, (lo, hi) in enumerate(ref['segs']):
        sp, sn, sloc = ref['scales'][i]
        sel = slice(lo, hi)
        pp, mm = ref['pos'][sel], ref['mined'][sel]
        blk = b_cls[sel]
        if pp.any():
            blk[pp] = gr._rows_bound(x[sel][pp], ref['labels'][sel][pp], sp, ref['softmax'][sel][pp])
        if mm.any():
            blk[mm] = gr._rows_bound(x[sel][mm], np.zeros(int(mm.sum()), np.int64), sn, ref['softmax'][sel][mm])
        s = abs(float(sloc))
        b_loc[sel][pp] = (s * U * np.where(d[sel][pp] < 1, d[sel][pp], 0.0) + 2 * U * np.minimum(d[sel][pp], 1.0) * s) * (1 + 1e-6) + TINY
    return b_cls, b_loc


def within(got, ref, bound):
    return gr.within(got, ref, bound)
