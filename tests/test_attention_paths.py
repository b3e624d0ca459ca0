"""Every kernel path behind the attention entry points -- egv_attn_fwd, egv_attn_bwd_dq, egv_attn_bwd_dkv, egv_attn_bwd_fused and
egv_attn_bwd_extra_reduce -- reached on purpose through a descriptor the case builds itself, and checked element by element against
fp64.

Each case names the path every call must take and the test asserts it (egv_attn_last_path: kind * 100 + tile instance).  The kinds:

    forward (egv_attn_fwd)                          dQ (egv_attn_bwd_dq)               dK / dV (egv_attn_bwd_dkv)
     1  many queries over <= 32 keys (fewkeys)      21  MFMA unsplit                   31  MFMA unsplit
     2  time groups + CLS query, combine            22  MFMA, CLS pair (keeps ws)      32  MFMA, CLS pair (keeps ws)
     3  space groups                                23  MFMA split + combine           33  MFMA split + reduce
     4  space groups + CLS query, combine           24  one query (attn1) + combine    34  one key (attn1) + reduce
     5  MFMA unsplit                                25  VALU unsplit                   35  VALU unsplit
     6  MFMA unsplit + CLS partials, combine        26  VALU split + combine           36  VALU split + reduce
     7  <= 32 queries over many keys (fewq)
     8  one query (attn1) split + combine           one-pass backward (egv_attn_bwd_fused; declines return 1, kind 0)
     9  MFMA split + combine                        41  fewkeys + reduce               45  space + CLS reduce
    10  VALU unsplit                                42  fewq + reduce                  46  generic fused kernel
    11  VALU split + combine                        43  time + CLS reduce              47  generic fused kernel + CLS reduce
                                                    44  space                          51  egv_attn_bwd_extra_reduce
The tile instance: the MFMA kernels' NT (2, 4, 14, 18 tiles of 16 other-side rows; 13 = the 13-live-tile form of 193..208 rows);
the space kernels' SPACE_DISPATCH instance, NT when exact and 50 + NT for the run-time row-count forms.  Paths are reached through
shape, stride, workspace, mask and O32 only: the EGV_ATTN_* switches are read once per process and stay at their defaults.

What every case checks:
  * the reference is fp64 divided / plain attention on the very inputs the kernel saw: the groups' queries over [CLS key ; group
    keys], the CLS query over [CLS ; every group's keys], with the additive key mask before the softmax.  Gradients of every row
    gather all its (query, key) pairs, so the CLS key row of dK / dV collects every group's queries and the CLS query;
  * element-wise first-order bound, from the kernels' arithmetic (constants below): logits carry the fp32 sum of 64 products
    (66 u |q||k| scaled), the fp32 rounding of scale * log2e and of s - max (4 u (|s| + |max|)) and the exp / exp2 error (2 u);
    that error goes through the softmax as p_j (e_j + sum p e); P.V and dS.K sums carry (n + 64) u of their absolute sums (n
    products and up to 64 rescalings, wave merges or partial-state merges in fp32); bf16 kernels that feed P and dS to an MFMA
    round them to bf16 (U_BF16 of each); delta carries the rounding of the O it was formed from (bf16 O, or fp32 O32); each output
    rounds once (U_BF16 / U_F32).  lse and delta are fp32 outputs with their own bounds;
  * the worst element is reported per region (CLS query row, CLS key row, first row of a group, last ragged 16-row tile, last
    sample, body) and a miss names its (b, g, h, row, column);
  * every output (O, O32, lse, delta, dQ, dK, dV) lives in a NaN-pattern buffer with a padded leading dimension, a non-zero head
    offset and guard rows; every element outside the rows and columns the call owns -- the CLS rows when it does not own them,
    the rows of a strided layout outside the row set -- must come back bit for bit;
  * a bf16 launch with O32 writes it within the fp32 bound, and O is O32 rounded to bf16, bit for bit;
  * two launches of every backward path give identical bits.
  * dropout cases check against keep_mult, a restatement of the kernels' counter hash; test_dropout_masks_agree reads the mask back
    through each dropout path's own forward (fewq, MFMA unsplit and split, VALU unsplit and split, bf16 and fp32) and requires it
    to equal keep_mult bit for bit;
  * the 2^31-byte offset gates of the time, space, fewkeys and fewq forwards: the gated matrix padded to just under and just over
    2 GB, so the last sample's rows sit at the largest offsets; the backward kernels' copies of these gates are not reached here.
"""
import math
import zlib

import pytest
import torch

gpu = pytest.mark.gpu

U = 2.0 ** -24              # fp32 arithmetic (one rounding)
U_BF16 = 2.0 ** -8          # bf16 output / MFMA-operand rounding (as tests/test_gemm_paths.py)
U_F32 = 2.0 ** -23          # fp32 output rounding
MERGES = 64                 # fp32 rescalings / wave merges / partial-state merges a sum may go through
CANARY = {torch.bfloat16: (torch.int16, 0x7FA5), torch.float32: (torch.int32, 0x7FA5A5A5)}
HD = 64
F32_MIN = torch.finfo(torch.float32).min     # the model's mask value (model.py)

PATHS = {
    100: 'fwd fewkeys', 200: 'fwd time + combine',
    313: 'fwd space nt13', 355: 'fwd space nt<5',
    403: 'fwd space+CLS nt3', 405: 'fwd space+CLS nt5', 413: 'fwd space+CLS nt13', 414: 'fwd space+CLS nt14', 417: 'fwd space+CLS nt17',
    455: 'fwd space+CLS nt<5', 463: 'fwd space+CLS nt6..12', 467: 'fwd space+CLS nt15..16',
    502: 'fwd MFMA NT2', 504: 'fwd MFMA NT4', 513: 'fwd MFMA 13 live', 514: 'fwd MFMA NT14', 518: 'fwd MFMA NT18',
    613: 'fwd MFMA+CLS 13 live', 614: 'fwd MFMA+CLS NT14',
    700: 'fwd fewq', 800: 'fwd attn1 split', 914: 'fwd MFMA split NT14', 918: 'fwd MFMA split NT18',
    1000: 'fwd VALU', 1100: 'fwd VALU split',
    2102: 'dq MFMA NT2', 2104: 'dq MFMA NT4', 2114: 'dq MFMA NT14', 2118: 'dq MFMA NT18', 2202: 'dq MFMA CLS pair',
    2302: 'dq MFMA split', 2400: 'dq attn1', 2500: 'dq VALU', 2600: 'dq VALU split',
    3102: 'dkv MFMA NT2', 3104: 'dkv MFMA NT4', 3114: 'dkv MFMA NT14', 3118: 'dkv MFMA NT18', 3202: 'dkv MFMA CLS pair',
    3302: 'dkv MFMA split', 3400: 'dkv attn1', 3500: 'dkv VALU', 3600: 'dkv VALU split',
    4100: 'fused fewkeys', 4200: 'fused fewq', 4300: 'fused time',
    4455: 'fused space nt<5', 4413: 'fused space nt13', 4514: 'fused space+CLS nt14', 4513: 'fused space+CLS nt13',
    4505: 'fused space+CLS nt5', 4503: 'fused space+CLS nt3', 4567: 'fused space+CLS nt15..16', 4563: 'fused space+CLS nt6..12',
    4600: 'fused generic', 4700: 'fused generic + CLS', 5100: 'extra reduce',
}
VALU = {8, 10, 11, 24, 25, 26, 34, 35, 36}      # kinds whose arithmetic is fp32 VALU throughout (no bf16 P / dS)


# ---------------------------------------------------------------- fp64 reference and bound (pure torch: runs on the CPU too)
def attn_reference(q, k, v, scale, madd=None, do=None, *, mfma=True, o_from32=False, u_out=U_BF16, keep=None):
    """fp64 attention of queries q [.., n, 64] over keys k, v [.., m, 64] with the additive key mask madd [.., m] (broadcast) and the
    first-order error bound of every output.  do: dO for the backward (dQ, dK, dV, delta).  mfma: the kernel rounds P and dS to bf16
    before its products.  o_from32: delta is formed from fp32 O32 (else from bf16 O).  u_out: the outputs' rounding.  keep: the dropout
    multiplier (0 or 1 / (1 - p)) of every probability, applied after the softmax.  Returns a dict of outputs and '<name>_b' bounds."""
    m = k.shape[-2]
    s = (q @ k.transpose(-1, -2)) * scale
    A = (q.abs() @ k.abs().transpose(-1, -2)) * abs(scale)
    if madd is not None:
        s = s + madd.unsqueeze(-2)
        A = A + madd.abs().unsqueeze(-2)
    mx = s.amax(-1, keepdim=True)
    p = torch.softmax(s, -1)
    lse = torch.logsumexp(s, -1)
    Es = 66 * U * A + 4 * U * (s.abs() + mx.abs()) + 2 * U                          # logit error: sum, scalings, exp
    Es = torch.where(p > 0, Es, torch.zeros_like(Es))                               # masked keys: p = 0 exactly in every path
    pe = (p * Es).sum(-1, keepdim=True)
    dp_f = p * (Es + pe)                                                            # softmax: p_j (e_j + sum p e)
    uP = U_BF16 if mfma else 0.0
    km = torch.ones_like(p) if keep is None else keep
    pt = p * km                                                                     # the probabilities P.V uses
    pv = pt @ v.abs()
    o = pt @ v
    acc = (m + MERGES) * U
    ob = (dp_f * km) @ v.abs() + (uP + acc) * pv + u_out * o.abs()
    out = dict(o=o, o_b=ob, lse=lse, lse_b=pe.squeeze(-1) + (m + MERGES) * U + 2 * U * (1 + lse.abs()) + U_F32 * lse.abs(), p=p)
    if do is None:
        return out
    # backward: p = exp(s - lse_in) with lse_in the fp32 rounding of lse
    dpb = p * (Es + 2 * U * lse.abs().unsqueeze(-1))
    dP = (do @ v.transpose(-1, -2)) * km
    dPb = 66 * U * (do.abs() @ v.abs().transpose(-1, -2)) * km
    delta = (do * o).sum(-1)
    uO = U_F32 if o_from32 else U_BF16
    ob = ob - u_out * o.abs() + U_BF16 * o.abs()    # the O the backward reads
    db = ((do.abs() * o.abs()).sum(-1) * (uO + 66 * U) + (dpb * dP.abs()).sum(-1) + (m + MERGES) * U * (p * dP.abs()).sum(-1)
          + (do.abs() * ob).sum(-1))
    ds = p * (dP - delta.unsqueeze(-1))
    uS = U_BF16 if mfma else 0.0
    dsb = dpb * (dP - delta.unsqueeze(-1)).abs() + p * (dPb + db.unsqueeze(-1)) + (uS + 2 * U) * ds.abs()
    dq = (ds @ k) * scale
    dqb = (dsb @ k.abs() + acc_n(m) * (ds.abs() @ k.abs())) * abs(scale) + u_out * dq.abs()
    n = q.shape[-2]
    dk = (ds.transpose(-1, -2) @ q) * scale
    dkb = (dsb.transpose(-1, -2) @ q.abs() + acc_n(n) * (ds.abs().transpose(-1, -2) @ q.abs())) * abs(scale) + u_out * dk.abs()
    dv = pt.transpose(-1, -2) @ do
    dvb = ((dpb + uP * p) * km).transpose(-1, -2) @ do.abs() + acc_n(n) * (pt.transpose(-1, -2) @ do.abs()) + u_out * dv.abs()
    out.update(dq=dq, dq_b=dqb, dk=dk, dk_b=dkb, dv=dv, dv_b=dvb, delta=delta, delta_b=db + U_F32 * delta.abs())
    return out


def acc_n(n):
    return (n + MERGES) * U


def region_report(out, ref, bound, labels, where):
    """Worst |out - ref| / bound per region.  out / ref / bound [R, C]; labels: region name per row; where(r, c) -> location text.
    Returns {region: (ratio, location, out, ref, bound)}; NaN / inf in out count as an infinite ratio."""
    out, ref, bound = out.double(), ref.double(), bound.double()
    err = (out - ref).abs()
    ratio = torch.where(err <= bound, err / bound.clamp_min(1e-300), torch.full_like(err, math.inf))
    ratio = torch.where(err == 0, torch.zeros_like(err), ratio).cpu()
    rep = {}
    for name in sorted(set(labels)):
        rows = torch.tensor([i for i, l in enumerate(labels) if l == name])
        r = ratio[rows]
        i = int(torch.argmax(r))
        ri, ci = int(rows[i // r.shape[1]]), i % r.shape[1]
        rep[name] = (float(r.view(-1)[i]), where(ri, ci), float(out[ri, ci]), float(ref[ri, ci]), float(bound[ri, ci]))
    return rep


def assert_within(what, out, ref, bound, labels, where):
    rep = region_report(out, ref, bound, labels, where)
    bad = {k: v for k, v in rep.items() if not v[0] <= 1.0}
    assert not bad, what + ': ' + '; '.join(f"{k}: worst at {v[1]} got {v[2]!r} want {v[3]!r} (bound {v[4]:.3g}, {v[0]:.3g}x)"
                                            for k, v in bad.items())
    return max((v[0] for v in rep.values()), default=0.0)


# ---------------------------------------------------------------- problem layouts
class Problem:
    """Row sets of one launch and the fp64 divided / plain attention over them.
    divided: tokens per sample S = 1 + F N, the CLS row first; 'space' groups = frames (rows 1 + f N + i), 'time' groups = patch
    positions (rows 1 + n + f N), the CLS row the extra row on the other side.  plain: queries b nq + i of Q, keys b nk + j of K / V."""

    def __init__(self, kind, B, H, F=0, N=0, nq=0, nk=0, groups=None, cls_last=False):
        self.kind, self.B, self.H = kind, B, H
        if kind == 'plain':
            self.G, self.nq, self.nk, self.extra = 1, nq, nk, 0
            self.q_rs, self.k_rs = (nq, 0, 0, 1), (nk, 0, 0, 1)
            self.q_rows, self.k_rows = B * nq, B * nk
            self.extra_bs = self.extra_row = 0
        else:
            S = 1 + F * N
            self.S, self.extra, self.extra_bs = S, 1, S
            self.extra_row, base = (F * N, 0) if cls_last else (0, 1)      # the CLS row first, or after the patches
            if kind == 'space':
                self.G, n, rs = F, N, (S, base, N, 1)
            else:                                                           # groups < N: rows of the other patch positions unused
                self.G, n, rs = (groups or N), F, (S, base, 1, N)
            self.nq = self.nk = n
            self.q_rs = self.k_rs = rs
            self.q_rows = self.k_rows = B * S

    def rows(self, rs, n):
        bs, base, gs, is_ = rs
        b = torch.arange(self.B).view(-1, 1, 1)
        g = torch.arange(self.G).view(1, -1, 1)
        i = torch.arange(n).view(1, 1, -1)
        return b * bs + base + g * gs + i * is_                                     # [B, G, n]

    def qidx(self):
        return self.rows(self.q_rs, self.nq)

    def kidx(self):
        return self.rows(self.k_rs, self.nk)

    def cls_rows(self):
        return torch.arange(self.B) * self.extra_bs + self.extra_row

    def labels(self, idx, cls_label):
        """region per row (owned rows in idx order [B, G, n] then the CLS rows when cls_label) and (b, g, i) of each"""
        labs, meta = [], []
        n = idx.shape[-1]
        last_tile = (n - 1) // 16 * 16 if n % 16 else n
        for b in range(self.B):
            for g in range(self.G):
                for i in range(n):
                    lab = 'first row of a group' if i == 0 else ('last ragged tile' if i >= last_tile else
                                                                  ('last sample' if b == self.B - 1 else 'body'))
                    labs.append(lab)
                    meta.append((b, g, i, int(idx[b, g, i])))
        if cls_label:
            for b in range(self.B):
                labs.append(cls_label)
                meta.append((b, -1, -1, int(self.cls_rows()[b])))
        return labs, meta


def heads(x, idx, off, H):
    """x [rows, ld] -> fp64 [.., H, n, 64] of the rows idx [.., n]"""
    t = x[:, off:off + H * HD][idx.to(x.device)].double()
    return t.unflatten(-1, (H, HD)).movedim(-2, -3)


def _mul32(a, c):
    """(a * c) mod 2^32 for 0 <= a, c < 2^32 without leaving int64"""
    return (((a & 0xFFFF) * c) + ((((a >> 16) * c) & 0xFFFF) << 16)) & 0xFFFFFFFF


def _fmix32(h):
    h = h ^ (h >> 16)
    h = _mul32(h, 0x85EBCA6B)
    h = h ^ (h >> 13)
    h = _mul32(h, 0xC2B2AE35)
    return h ^ (h >> 16)


def keep_mult(P, p, seed):
    """The dropout multiplier drop_mult (egv_attn.h) gives every (query, key, head) of a plain launch: [B, G, H, nq, nk] fp64, 0 or
    fp32(1 / (1 - p)).  The counter hash of (seed, row-set query index, key index, head), restated in 64-bit integers."""
    M32 = 0xFFFFFFFF
    b = torch.arange(P.B, dtype=torch.int64).view(-1, 1, 1, 1, 1)
    g = torch.arange(P.G, dtype=torch.int64).view(1, -1, 1, 1, 1)
    h = torch.arange(P.H, dtype=torch.int64).view(1, 1, -1, 1, 1)
    i = torch.arange(P.nq, dtype=torch.int64).view(1, 1, 1, -1, 1)
    j = torch.arange(P.nk, dtype=torch.int64).view(1, 1, 1, 1, -1)
    qrow = (b * P.G + g) * P.nq + i
    x = seed ^ _fmix32((_mul32(qrow & M32, 0x9E3779B1) + h) & M32)
    x = _fmix32(x ^ ((_mul32(j & M32, 0x85EBCA77) + 0x165667B1) & M32))
    u = (x >> 8).double() * 2.0 ** -24                                  # exact in fp32 too
    pf = float(torch.tensor(p, dtype=torch.float32))
    inv = float(1.0 / torch.tensor(1.0 - pf, dtype=torch.float32))      # fp32 1 / (1 - p)
    return torch.where(u >= pf, torch.full_like(u, inv), torch.zeros_like(u))


def full_reference(P, Q, K, V, qoff, koff, voff, scale, mask=None, dO=None, ooff=0, mfma=True, o_from32=False, u_out=U_BF16,
                   keep=None):
    """Reference outputs per row of the token matrices: O, lse (query rows), dQ, delta (query rows), dK, dV (key rows).
    Returns dict name -> (value [rows, H, 64] or [rows, H], bound) indexed by token row (rows nobody owns stay 0)."""
    H, dev = P.H, Q.device
    qi, ki = P.qidx(), P.kidx()
    q, k, v = heads(Q, qi, qoff, H), heads(K, ki, koff, H), heads(V, ki, voff, H)       # [B, G, H, n, 64]
    madd = None
    if mask is not None:
        madd = mask.double()[:, :P.nk].view(P.B, 1, 1, P.nk)
    do = heads(dO, qi, ooff, H) if dO is not None else None
    if P.extra:
        cr = P.cls_rows().view(P.B, 1, 1)
        kc, vc = heads(K, cr, koff, H), heads(V, cr, voff, H)                             # [B, 1, H, 1, 64]
        kx = torch.cat([kc.expand(-1, P.G, -1, -1, -1), k], -2)
        vx = torch.cat([vc.expand(-1, P.G, -1, -1, -1), v], -2)
        assert madd is None
    else:
        kx, vx = k, v
    assert keep is None or not P.extra
    R = attn_reference(q, kx, vx, scale, madd, do, mfma=mfma, o_from32=o_from32, u_out=u_out, keep=keep)
    rows_q, rows_k = P.q_rows, P.k_rows
    out = {}

    def put(name, rows, idx, val, bnd, last_dim=True):
        shape = (rows, H, HD) if last_dim else (rows, H)
        if name not in out:
            out[name] = [torch.zeros(shape, dtype=torch.float64, device=dev), torch.zeros(shape, dtype=torch.float64, device=dev)]
        idx = idx.reshape(-1).to(dev)
        if last_dim:
            val, bnd = val.movedim(-3, -2).reshape(-1, H, HD), bnd.movedim(-3, -2).reshape(-1, H, HD)
        else:
            val, bnd = val.movedim(-2, -1).reshape(-1, H), bnd.movedim(-2, -1).reshape(-1, H)
        out[name][0].index_add_(0, idx, val)
        out[name][1].index_add_(0, idx, bnd)

    put('o', rows_q, qi, R['o'], R['o_b'])
    put('lse', rows_q, qi, R['lse'], R['lse_b'], False)
    if do is not None:
        put('dq', rows_q, qi, R['dq'], R['dq_b'])
        put('delta', rows_q, qi, R['delta'], R['delta_b'], False)
        kpart = lambda t: t[..., P.extra:, :]            # noqa: E731
        put('dk', rows_k, ki, kpart(R['dk']), kpart(R['dk_b']))
        put('dv', rows_k, ki, kpart(R['dv']), kpart(R['dv_b']))
        if P.extra:                                      # the CLS key under every group's queries
            put('dk', rows_k, cr.expand(-1, P.G, 1), R['dk'][..., :1, :], R['dk_b'][..., :1, :])
            put('dv', rows_k, cr.expand(-1, P.G, 1), R['dv'][..., :1, :], R['dv_b'][..., :1, :])
    if P.extra:                                          # the CLS query over [CLS ; every group's keys]
        qc = heads(Q, P.cls_rows().view(P.B, 1), qoff, H)                                 # [B, H, 1, 64]
        kall = torch.cat([kc[:, 0], k.movedim(1, 2).reshape(P.B, H, P.G * P.nk, HD)], -2)
        vall = torch.cat([vc[:, 0], v.movedim(1, 2).reshape(P.B, H, P.G * P.nk, HD)], -2)
        doc = heads(dO, P.cls_rows().view(P.B, 1), ooff, H) if dO is not None else None
        C = attn_reference(qc, kall, vall, scale, None, doc, mfma=mfma, o_from32=o_from32, u_out=u_out)
        cr1 = P.cls_rows().view(P.B, 1)
        put('o', rows_q, cr1, C['o'], C['o_b'])
        put('lse', rows_q, cr1, C['lse'], C['lse_b'], False)
        if doc is not None:
            put('dq', rows_q, cr1, C['dq'], C['dq_b'])
            put('delta', rows_q, cr1, C['delta'], C['delta_b'], False)
            gk = ki.view(P.B, 1, P.G * P.nk)
            put('dk', rows_k, gk, C['dk'][..., 1:, :], C['dk_b'][..., 1:, :])
            put('dv', rows_k, gk, C['dv'][..., 1:, :], C['dv_b'][..., 1:, :])
            put('dk', rows_k, cr1, C['dk'][..., :1, :], C['dk_b'][..., :1, :])
            put('dv', rows_k, cr1, C['dv'][..., :1, :], C['dv_b'][..., :1, :])
    return out


# ---------------------------------------------------------------- self-tests of the checker and the path table (no GPU)
def _small_divided(gen, B=2, H=2, F=3, N=21):
    P = Problem('space', B, H, F=F, N=N)
    D = 3 * H * HD
    X = (torch.randn(P.q_rows, D, generator=gen)).to(torch.bfloat16)
    dO = (torch.randn(P.q_rows, H * HD, generator=gen)).to(torch.bfloat16)
    return P, X, dO


def _rows_check(name, got, ref, bnd, P, rows_idx, labels):
    meta = labels[1]
    H = P.H
    g = got[rows_idx].reshape(len(rows_idx), -1)
    r, b = ref[rows_idx].reshape(len(rows_idx), -1), bnd[rows_idx].reshape(len(rows_idx), -1)
    cols = g.shape[1]
    per_h = cols // H

    def where(ri, ci):
        bb, gg, ii, row = meta[ri]
        return f"(b={bb}, g={gg}, h={ci // per_h}, row={row}, col={ci % per_h})"
    return assert_within(name, g, r, b, labels[0], where)


def test_checker_rejects_cls_ulps_ragged_shift_swapped_heads_and_lse():
    """The bound passes the exactly rounded reference and rejects: 2 bf16 ulps in one CLS-row element, the last ragged tile shifted
    by one row, two heads swapped, an lse off by 1e-3 -- each named in its region."""
    gen = torch.Generator().manual_seed(11)
    P, X, dO = _small_divided(gen)
    H = P.H
    R = full_reference(P, X, X, X, 0, H * HD, 2 * H * HD, 0.125, dO=dO, mfma=False)   # the fp32-P (VALU) bound
    o, ob = R['o']
    qi = P.qidx()
    labels = P.labels(qi, 'CLS query row')
    rows_idx = torch.cat([qi.reshape(-1), P.cls_rows()])
    good = o.to(torch.bfloat16).double()
    _rows_check('exact', good, o, ob, P, rows_idx, labels)
    # 2 ulps in one element of the first CLS row
    bad = good.clone()
    c = P.cls_rows()[0]
    x = bad[c, 1, 5]
    ulp = 2.0 ** (math.floor(math.log2(abs(float(x)))) - 7)
    bad[c, 1, 5] = x + 2 * ulp
    with pytest.raises(AssertionError, match=r'CLS query row: worst at \(b=0, g=-1, h=1, row=0, col=5\)'):
        _rows_check('cls', bad, o, ob, P, rows_idx, labels)
    # the last ragged tile (rows 16..20 of each group) shifted by one row
    bad = good.clone()
    rg = qi[1, 2]
    bad[rg[16:]] = good[torch.cat([rg[17:], rg[16:17]])]
    with pytest.raises(AssertionError, match='last ragged tile'):
        _rows_check('shift', bad, o, ob, P, rows_idx, labels)
    # two heads swapped
    bad = good.clone()
    bad[:, [0, 1]] = good[:, [1, 0]]
    with pytest.raises(AssertionError, match='body'):
        _rows_check('heads', bad, o, ob, P, rows_idx, labels)
    # lse off by 1e-3 in one row of the last sample
    lse, lseb = R['lse']
    lg = lse.float().double()
    _rows_check('lse exact', lg, lse, lseb, P, rows_idx, labels)
    lbad = lg.clone()
    lbad[qi[1, 0, 7], 0] += 1e-3
    with pytest.raises(AssertionError, match=r'last sample: worst at \(b=1, g=0, h=0'):
        _rows_check('lse', lbad, lse, lseb, P, rows_idx, labels)


# ---------------------------------------------------------------- cases
@pytest.fixture(scope='module')
def ops():
    from egovlpv2_amd import hipops
    return hipops


def C(name, paths, **kw):
    return pytest.param(dict(paths=paths, **kw), id=name)


# layout: ('space' | 'time', B, H, F, N) or ('plain', B, H, nq, nk).  op: 'fwd', 'dq', 'dkv', 'pair' (dq + dkv with the CLS pair
# workspace + extra_reduce), 'fused', 'split' (dq + dkv with nsplit).  paths: the codes the calls must record, in order.
FWD_CASES = [
    # space: groups with CLS through the workspace, every SPACE_DISPATCH instance; groups only
    C('space_nt2_cls', [455], lay=('space', 2, 2, 3, 17), cls_ws=True),
    C('space_nt3_cls', [403], lay=('space', 2, 2, 3, 33), cls_ws=True),
    C('space_nt4_cls', [455], lay=('space', 1, 2, 2, 49), cls_ws=True),
    C('space_nt5_cls', [405], lay=('space', 3, 2, 2, 65), cls_ws=True),
    C('space_nt6_cls', [463], lay=('space', 2, 2, 2, 81), cls_ws=True),
    C('space_nt12_cls', [463], lay=('space', 1, 2, 2, 191), cls_ws=True),
    C('space_nt13_cls_base', [413], lay=('space', 2, 12, 4, 196), cls_ws=True),
    C('space_nt14_cls', [414], lay=('space', 2, 2, 3, 209), cls_ws=True),
    C('space_nt15_cls', [467], lay=('space', 1, 2, 2, 225), cls_ws=True),
    C('space_nt17_cls', [417], lay=('space', 2, 2, 2, 256), cls_ws=True),
    C('space_nt13_groups', [313], lay=('space', 2, 2, 4, 196)),
    C('space_nt2_groups', [355], lay=('space', 3, 2, 2, 17)),
    C('space_vitl_fr16', [413], lay=('space', 1, 16, 16, 196), cls_ws=True, ld_pad=8, ooff=8),
    # Q, K, V not slices of one buffer: space declines, the MFMA kernel with CLS partials takes it
    C('space_leaves_separate_qkv', [613], lay=('space', 2, 2, 4, 196), cls_ws=True, separate=True),
    C('mfma_cls_nt14', [614], lay=('space', 2, 2, 3, 150), cls_ws=True, separate=True),
    C('space_leaves_ld_mod8', [1000], lay=('space', 2, 2, 4, 196), cls_ws=True, ld_pad=4),
    # time: <= 16-row groups with the CLS query, production frame counts
    C('time_fr4', [200], lay=('time', 2, 12, 4, 196), cls_ws=True),
    C('time_fr16', [200], lay=('time', 3, 2, 16, 49), cls_ws=True),
    C('time_fr16_ws_short', [502], lay=('time', 2, 2, 16, 49), cls_ws=True, ws_short=4),
    C('time_fr32', [403], lay=('time', 1, 2, 32, 49), cls_ws=True),
    C('time_leaves_ldo_mod8', [1000], lay=('time', 2, 2, 4, 49), cls_ws=True, ldo_pad=4),
    # MFMA unsplit, each instance, groups only (no workspace: the CLS query is the caller's)
    C('mfma_nt2_plain', [502], lay=('plain', 3, 2, 40, 32)),
    C('mfma_nt4_plain', [504], lay=('plain', 1, 2, 33, 64)),
    C('mfma_nt14_plain', [514], lay=('plain', 2, 2, 100, 150)),
    C('mfma_nt13_plain', [513], lay=('plain', 2, 2, 70, 197)),
    C('mfma_nt18_plain', [518], lay=('plain', 2, 2, 50, 288)),
    C('mfma_nt18_masked_tile', [518], lay=('plain', 2, 2, 50, 288), mask='tile'),
    C('mfma_nt14_mask_1e4', [514], lay=('plain', 2, 2, 100, 150), mask='1e4'),
    C('mfma_leaves_289', [1000], lay=('plain', 2, 2, 20, 289)),
    C('mfma_leaves_ldq_mod8', [1000], lay=('plain', 2, 2, 40, 100), ld_pad=4),
    # fewkeys: >= 128 queries over <= 32 keys (the i2t shape with its padded text mask)
    C('fewkeys_i2t', [100], lay=('plain', 2, 12, 3137, 32), mask='text', mask_ld=40),
    C('fewkeys_q513', [100], lay=('plain', 3, 2, 513, 20)),
    C('fewkeys_leaves_k33', [504], lay=('plain', 2, 2, 200, 33)),
    C('fewkeys_leaves_q127', [502], lay=('plain', 2, 2, 127, 32)),
    C('fewkeys_leaves_o32', [502], lay=('plain', 2, 2, 200, 32), o32=True),
    # fewq: <= 32 queries over >= 512 keys (t2i), with the combination
    C('fewq_t2i', [700], lay=('plain', 2, 12, 32, 3137), fewq_ws=True, o32=True),
    C('fewq_k512_o32', [700], lay=('plain', 1, 2, 7, 512), fewq_ws=True, o32=True),
    C('fewq_k769', [700], lay=('plain', 3, 2, 32, 769), fewq_ws=True),
    C('fewq_leaves_k511', [1000], lay=('plain', 2, 2, 8, 511), fewq_ws=True),
    C('fewq_leaves_q33', [1000], lay=('plain', 2, 2, 33, 600), fewq_ws=True),
    C('fewq_leaves_ws_short', [1000], lay=('plain', 2, 2, 8, 600), fewq_ws=True, ws_short=4),
    C('fewq_leaves_mask', [1000], lay=('plain', 2, 2, 8, 600), fewq_ws=True, mask='1e4'),
    # split forms + combination
    C('attn1_split_cls_query', [800], lay=('plain', 3, 2, 1, 785), nsplit=4, o32=True),
    C('mfma_split', [914], lay=('plain', 2, 2, 20, 400), nsplit=2, o32=True),
    C('mfma_split_mask_chunk', [918], lay=('plain', 2, 2, 20, 500), nsplit=2, mask='chunk'),
    C('valu_split_o32', [1100], lay=('plain', 2, 2, 70, 600), nsplit=3, o32=True),
    C('valu_split_f32', [1100], lay=('plain', 2, 2, 70, 600), nsplit=3, dt='f32'),
    # VALU unsplit: fp32, and bf16 where MFMA declines (the O32 contract)
    C('valu_f32_masked', [1000], lay=('plain', 2, 2, 45, 100), dt='f32', mask='min'),
    C('valu_o32_ld_mod8', [1000], lay=('plain', 2, 2, 40, 100), ld_pad=4, o32=True),
    C('valu_o32_289_keys', [1000], lay=('plain', 1, 2, 20, 300), o32=True),
    C('mfma_nt14_o32', [514], lay=('plain', 2, 2, 100, 150), o32=True),
    # offsets 4 (mod 8): the MFMA and fewkeys kernels decline, the VALU kernel takes the call
    C('valu_ooff4', [1000], lay=('plain', 2, 2, 40, 100), ooff=4),
    C('fewkeys_leaves_ooff4', [1000], lay=('plain', 2, 2, 200, 32), ooff=4),
    C('fewkeys_q128', [100], lay=('plain', 2, 2, 128, 32)),
    # a strided time layout whose row set leaves the rows of 19 patch positions alone
    C('time_fr16_30_groups', [200], lay=('time', 2, 2, 16, 49), cls_ws=True, groups=30),
    # attention dropout (p = 0.25) on every forward path that takes it
    C('drop_mfma_nt14', [514], lay=('plain', 2, 2, 100, 150), drop=0.25),
    C('drop_mfma_nt2_mask', [502], lay=('plain', 3, 2, 40, 32), drop=0.25, mask='min'),
    C('drop_mfma_split', [918], lay=('plain', 2, 2, 20, 500), nsplit=2, drop=0.25),
    C('drop_fewq', [700], lay=('plain', 2, 2, 32, 600), fewq_ws=True, drop=0.25, o32=True),
    C('drop_valu', [1000], lay=('plain', 2, 2, 40, 100), ld_pad=4, drop=0.25),
    C('drop_valu_split_f32', [1100], lay=('plain', 2, 2, 70, 600), nsplit=3, dt='f32', drop=0.25),
    # the 2^31-byte offset limit: the gated matrix just under (the kernel takes it) and just over (the fallback); its last rows are
    # those of the last sample, where a wrapped 32-bit offset would land
    C('big_space_in', [413], lay=('space', 2, 2, 4, 196), cls_ws=True, big='in'),
    C('big_space_out', [613], lay=('space', 2, 2, 4, 196), cls_ws=True, big='out'),
    C('big_time_in', [200], lay=('time', 2, 2, 16, 49), cls_ws=True, big='in'),
    C('big_time_out', [502], lay=('time', 2, 2, 16, 49), cls_ws=True, big='out'),
    C('big_fewkeys_in', [100], lay=('plain', 2, 2, 200, 32), big='in', big_side='q'),
    C('big_fewkeys_out', [502], lay=('plain', 2, 2, 200, 32), big='out', big_side='q'),
    C('big_fewq_in', [700], lay=('plain', 2, 2, 8, 600), fewq_ws=True, big='in', big_side='k'),
    C('big_fewq_out', [1000], lay=('plain', 2, 2, 8, 600), fewq_ws=True, big='out', big_side='k'),
    # O32 turns the time / space kernels away: the MFMA kernel (with CLS partials where it covers them) writes it
    C('space_o32_leaves', [613], lay=('space', 2, 2, 4, 196), cls_ws=True, o32=True),
    C('time_o32_leaves', [502], lay=('time', 2, 2, 4, 49), cls_ws=True, o32=True),
]


def _fill(shape, gen, scale=1.0, dt=torch.bfloat16):
    return (torch.randn(shape, generator=gen, device='cuda') * scale).to(dt)


class Buf:
    """[rows, ld] matrix inside a NaN-pattern buffer with guard rows; untouched(rows, c0, c1) checks every element outside rows x
    [c0, c1) kept its bits."""

    def __init__(self, rows, ld, dtype, guard=2):
        itype, self.pat = CANARY[dtype]
        self.raw = torch.full(((rows + guard) * ld,), self.pat, dtype=itype, device='cuda')
        self.m = self.raw.view(dtype)[:rows * ld].view(rows, ld)
        self.ld = ld

    def ptr(self):
        return self.m.data_ptr()

    def untouched(self, rows, c0, c1):
        keep = torch.ones_like(self.raw, dtype=torch.bool)
        r = rows.to(self.raw.device).view(-1, 1)
        cols = torch.arange(c0, c1, device=self.raw.device).view(1, -1)
        keep[(r * self.ld + cols).reshape(-1)] = False
        return bool((self.raw[keep] == self.pat).all())


def _mask_for(kind, B, nk, ld, gen):
    if kind is None:
        return None
    m = torch.zeros(B, ld, dtype=torch.float32, device='cuda')
    if kind == 'zero':                                    # a mask that masks nothing (the fewq kernel declines any mask)
        return m
    val = -10000.0 if kind == '1e4' else F32_MIN
    if kind in ('text', 'min', '1e4'):                    # padded text: per sample a valid length, the CLS key always kept
        for b in range(B):
            L = max(1, nk - 3 - 5 * b)
            m[b, L:nk] = val
    elif kind == 'tile':                                  # a whole 16-key tile masked
        m[:, 16:32] = val
        m[1:, nk - 40:nk] = val
    elif kind == 'chunk':                                 # the whole second split chunk of sample 0
        m[0, nk // 2:nk] = val
    m[:, nk:] = float('nan')                              # beyond k_n: never read
    return m


def _setup(ops, c):
    L = ops.L
    gen = torch.Generator(device='cuda').manual_seed(zlib.crc32(repr(sorted((k, str(v)) for k, v in c.items())).encode()))
    lay = c['lay']
    P = (Problem(lay[0], lay[1], lay[2], F=lay[3], N=lay[4], groups=c.get('groups'), cls_last=c.get('cls_last', False))
         if lay[0] != 'plain' else Problem('plain', lay[1], lay[2], nq=lay[3], nk=lay[4]))
    H = P.H
    dt = torch.float32 if c.get('dt') == 'f32' else torch.bfloat16
    pad = c.get('ld_pad', 0)
    big = c.get('big')               # 'in' / 'out': the gated matrix padded to just under / just over 2^31 bytes

    def mat(rows, used, ld, gated):
        if big and gated:
            lim = 1 << 31
            ld = ((lim - 1) // (2 * rows)) // 8 * 8 if big == 'in' else (-(-lim // (2 * rows)) + 7) // 8 * 8
            assert (rows * ld * 2 < lim) == (big == 'in')
            x = torch.zeros((rows, ld), dtype=dt, device='cuda')
            x[:, :used] = _fill((rows, used), gen, 1.0, dt)
            return x, ld
        return _fill((rows, ld), gen, 1.0, dt), ld
    if P.kind == 'plain':
        Q, ldq = mat(P.q_rows, H * HD, H * HD + pad, c.get('big_side') == 'q')
        KV, ldk = mat(P.k_rows, 2 * H * HD, 2 * H * HD + pad, c.get('big_side') == 'k')
        Qp, Kp, Vp, qoff, koff, voff = Q, KV, KV, 0, 0, H * HD
        ldv = ldk
    elif c.get('separate'):
        ldq = ldk = ldv = H * HD + pad
        Qp, Kp, Vp = (_fill((P.q_rows, ldq), gen, 1.0, dt) for _ in range(3))
        qoff = koff = voff = 0
    else:
        Qp, ldq = mat(P.q_rows, 3 * H * HD, 3 * H * HD + pad, True)
        ldk = ldv = ldq
        Kp = Vp = Qp
        qoff, koff, voff = 0, H * HD, 2 * H * HD
    ooff = c.get('ooff', 0)
    ldo = H * HD + ooff + 8 + c.get('ldo_pad', 0)
    mask_ld = c.get('mask_ld', P.nk)
    mask = _mask_for(c.get('mask'), P.B, P.nk, mask_ld, gen)
    d = L.AttnDesc()
    d.Q, d.K, d.V = Qp.data_ptr(), Kp.data_ptr(), Vp.data_ptr()
    d.ldq, d.ldk, d.ldv, d.ldo = ldq, ldk, ldv, ldo
    d.qoff, d.koff, d.voff, d.ooff = qoff, koff, voff, ooff
    d.B, d.G, d.H = P.B, P.G, H
    d.q_bs, d.q_base, d.q_gs, d.q_is = P.q_rs
    d.k_bs, d.k_base, d.k_gs, d.k_is = P.k_rs
    d.q_n, d.k_n = P.nq, P.nk
    d.extra, d.extra_bs, d.extra_row = P.extra, P.extra_bs, P.extra_row
    d.scale = 0.125
    d.mask, d.mask_ld = (mask.data_ptr(), mask_ld) if mask is not None else (None, 0)
    d.nsplit = c.get('nsplit', 1)
    if c.get('drop'):
        d.drop_p, d.drop_seed = c['drop'], c.get('seed', 1234)
    return P, dt, d, (Qp, Kp, Vp, qoff, koff, voff, ooff, ldo), mask, gen


def _ws(ops, c, P, d, which):
    lib = ops.lib
    nb = 0
    if d.nsplit > 1:
        nb = lib.egv_attn_split_workspace_bytes(which, P.B, P.G, P.H, P.nk if which == 2 else P.nq, d.nsplit)
        if which == 2:
            nb = lib.egv_attn_bwd_dkv_workspace_bytes(P.B, P.G, P.H, P.nk, d.nsplit)
    if c.get('cls_ws'):
        nb = max(nb, lib.egv_attn_fwd_extra_workspace_bytes(P.B, P.G, P.H))
    if c.get('fewq_ws'):
        nb = max(nb, lib.egv_attn_fewq_workspace_bytes(P.B, P.G, P.H, P.nk))
    if c.get('fewkeys_ws'):
        nb = max(nb, lib.egv_attn_fewkeys_workspace_bytes(P.B, P.G, P.H, P.nq))
    if c.get('bwd_ws'):
        nb = max(nb, lib.egv_attn_bwd_fused_workspace_bytes(P.B, P.G, P.H), lib.egv_attn_fewkeys_workspace_bytes(P.B, P.G, P.H, P.nq),
                 lib.egv_attn_fewq_workspace_bytes(P.B, P.G, P.H, P.nk))
    if nb == 0:
        return None
    nb -= c.get('ws_short', 0)
    ws = torch.full((nb // 4 + 1,), float('nan'), dtype=torch.float32, device='cuda')
    d.ws, d.ws_bytes = ws.data_ptr(), nb
    return ws


def _owned_q(P, cls_owned):
    qi = P.qidx()
    rows = torch.cat([qi.reshape(-1), P.cls_rows()]) if cls_owned else qi.reshape(-1)
    return qi, rows, P.labels(qi, 'CLS query row' if cls_owned else None)


def _check_rows(name, buf_m, R, rows, labels, P, width):
    ref, bnd = R
    got = buf_m[rows.to(buf_m.device)]
    g = got.reshape(len(rows), -1)
    r, b = ref[rows].reshape(len(rows), -1), bnd[rows].reshape(len(rows), -1)
    meta = labels[1]

    def where(ri, ci):
        bb, gg, ii, row = meta[ri]
        return f"(b={bb}, g={gg}, h={ci // width}, row={row}, col={ci % width})"
    return assert_within(name, g, r, b, labels[0], where)


RATIOS = {}


@pytest.fixture(scope='module', autouse=True)
def ratio_report(request):
    """After the module: the worst error-to-bound ratio each path reached over its cases (shown with -s or in the captured log)"""
    yield
    if RATIOS:
        lines = [f"  {p:5d} {PATHS.get(p, 'decline'):28s} {r:.3f}" for p, r in sorted(RATIOS.items())]
        capman = request.config.pluginmanager.getplugin('capturemanager')
        with capman.global_and_fixture_disabled():
            print('\nworst |kernel - fp64| / bound per attention path:\n' + '\n'.join(lines))


@gpu
@pytest.mark.parametrize('case', FWD_CASES)
def test_forward_path(ops, case):
    lib = ops.lib
    c = dict(case)
    P, dt, d, (Qp, Kp, Vp, qoff, koff, voff, ooff, ldo), mask, gen = _setup(ops, c)
    H = P.H
    ws = _ws(ops, c, P, d, 0)
    O = Buf(P.q_rows, ldo, dt)
    lse = Buf(P.q_rows, H, torch.float32)
    O32 = Buf(P.q_rows, ldo, torch.float32) if c.get('o32') else None
    d.O, d.lse = O.ptr(), lse.ptr()
    d.O32 = O32.ptr() if O32 is not None else None
    Ldt = ops.L.EGV_F32 if dt == torch.float32 else ops.L.EGV_BF16
    covers = bool(P.extra and d.ws and lib.egv_attn_fwd_covers_extra(Ldt, d))
    rc = lib.egv_attn_fwd(Ldt, d, ops._st())
    ops.check(rc, 'egv_attn_fwd')
    path = ops.attn_last_path()
    torch.cuda.synchronize()
    assert [path] == c['paths'], f"ran path {path} ({PATHS.get(path)}), the case says {c['paths']}"
    kind = path // 100
    if P.extra and c.get('cls_ws') and not c.get('ws_short'):
        assert covers == (kind in (2, 4, 6)), 'egv_attn_fwd_covers_extra disagrees with the path taken'
    if c.get('ws_short'):
        assert not covers, 'a workspace 4 bytes short covers nothing'
    cls_owned = kind in (2, 4, 6)
    keep = keep_mult(P, d.drop_p, d.drop_seed).cuda() if c.get('drop') else None
    R = full_reference(P, Qp, Kp, Vp, qoff, koff, voff, 0.125, mask=mask, mfma=(dt == torch.bfloat16 and kind not in VALU),
                       u_out=U_BF16 if dt == torch.bfloat16 else U_F32, keep=keep)
    qi, rows, labels = _owned_q(P, cls_owned)
    worst = _check_rows('O', O.m[:, ooff:ooff + H * HD].double().view(P.q_rows, H, HD), R['o'], rows, labels, P, HD)
    worst = max(worst, _check_rows('lse', lse.m.double(), R['lse'], rows, labels, P, 1))
    assert O.untouched(rows, ooff, ooff + H * HD), 'O: a write outside the owned rows / head columns'
    assert lse.untouched(rows, 0, H), 'lse: a write outside the owned rows'
    if O32 is not None:
        o32b = (R['o'][0], R['o'][1] - U_BF16 * R['o'][0].abs() + U_F32 * R['o'][0].abs())
        worst = max(worst, _check_rows('O32', O32.m[:, ooff:ooff + H * HD].view(P.q_rows, H, HD), o32b, rows, labels, P, HD))
        assert O32.untouched(rows, ooff, ooff + H * HD), 'O32: a write outside the owned rows / head columns'
        r = rows.cuda()
        assert torch.equal(O.m[r, ooff:ooff + H * HD], O32.m[r, ooff:ooff + H * HD].to(torch.bfloat16)), 'O is not O32 rounded to bf16'
    RATIOS[path] = max(RATIOS.get(path, 0.0), worst)


BWD_CASES = [
    # dQ + dK/dV pairs, each MFMA instance (plain) and the VALU fallbacks
    C('pair_nt2', [2102, 3102], lay=('plain', 2, 2, 30, 30), op='dqdkv'),
    C('pair_nt2_nt4', [2102, 3104], lay=('plain', 2, 2, 40, 30), op='dqdkv'),
    C('pair_nt4', [2104, 3104], lay=('plain', 3, 2, 50, 60), op='dqdkv'),
    C('pair_nt14_mask', [2114, 3114], lay=('plain', 2, 2, 100, 150), op='dqdkv', mask='min'),
    C('pair_nt18', [2118, 3118], lay=('plain', 2, 2, 280, 250), op='dqdkv', o32=True),
    C('pair_valu_289', [2500, 3500], lay=('plain', 2, 2, 300, 289), op='dqdkv', o32=True),
    C('pair_valu_ld_mod8', [2500, 3500], lay=('plain', 2, 2, 40, 100), op='dqdkv', ld_pad=4),
    C('pair_valu_f32', [2500, 3500], lay=('plain', 2, 2, 40, 100), op='dqdkv', dt='f32', mask='1e4'),
    # split forms
    C('split_mfma', [2302, 3302], lay=('plain', 2, 2, 20, 20), op='dqdkv', nsplit=2),
    C('split_attn1_q', [2400, 3600], lay=('plain', 2, 2, 1, 785), op='dqdkv', nsplit=4, o32=True),
    C('split_attn1_k', [2600, 3400], lay=('plain', 2, 2, 300, 1), op='dqdkv', nsplit=3, dt='f32'),
    C('split_valu', [2600, 3600], lay=('plain', 2, 2, 70, 600), op='dqdkv', nsplit=3),
    # the 17-row time pair: CLS partials + extra_reduce
    C('time_pair_cls', [2202, 3202, 5100], lay=('time', 2, 2, 16, 49), op='pair', bwd_ws=True),
    # one-pass backward
    C('fused_fewkeys_i2t', [4100], lay=('plain', 2, 12, 3137, 32), op='fused', bwd_ws=True, mask='text', mask_ld=40),
    C('fused_fewkeys_q513', [4100], lay=('plain', 3, 2, 513, 20), op='fused', bwd_ws=True),
    C('fused_fewq_t2i', [4200], lay=('plain', 2, 12, 32, 3137), op='fused', bwd_ws=True, o32=True),
    C('fused_fewq_k769', [4200], lay=('plain', 3, 2, 32, 769), op='fused', bwd_ws=True),
    C('fused_time_fr4', [4300], lay=('time', 2, 12, 4, 196), op='fused', bwd_ws=True),
    C('fused_time_fr16', [4300], lay=('time', 3, 2, 16, 49), op='fused', bwd_ws=True),
    C('fused_space_cls_nt13', [4513], lay=('space', 2, 12, 4, 196), op='fused', bwd_ws=True),
    C('fused_space_cls_nt14', [4514], lay=('space', 2, 2, 3, 209), op='fused', bwd_ws=True),
    C('fused_space_cls_nt5', [4505], lay=('space', 3, 2, 2, 65), op='fused', bwd_ws=True),
    C('fused_space_cls_nt3', [4503], lay=('time', 1, 2, 32, 49), op='fused', bwd_ws=True),
    C('fused_space_cls_nt6', [4563], lay=('space', 2, 2, 2, 81), op='fused', bwd_ws=True),
    C('fused_space_cls_nt15', [4567], lay=('space', 1, 2, 2, 225), op='fused', bwd_ws=True),
    C('fused_space_nt13', [4413], lay=('space', 2, 2, 4, 196), op='fused'),
    C('fused_space_nt2', [4455], lay=('space', 2, 2, 3, 17), op='fused'),
    C('fused_generic', [4600], lay=('space', 2, 2, 3, 196), op='fused', separate=True),
    C('fused_generic_cls', [4700], lay=('space', 2, 2, 3, 196), op='fused', bwd_ws=True, separate=True),
    # declines (return 1, nothing enqueued): the caller's dQ + dK/dV pair then runs
    C('fused_declines_f32', [0, 2500, 3500], lay=('plain', 2, 2, 100, 100), op='fused', dt='f32'),
    C('fused_declines_mask', [0, 2114, 3114], lay=('plain', 2, 2, 100, 100), op='fused', mask='1e4'),
    C('fused_declines_64_rows', [0, 2104, 3104], lay=('plain', 2, 2, 64, 64), op='fused'),
    C('fused_declines_o32', [0, 2114, 3114], lay=('space', 2, 2, 3, 100), op='fused', o32=True, separate=True),
    C('fused_declines_cls_last', [0, 2114, 3114], lay=('space', 2, 2, 3, 196), op='fused', bwd_ws=True, separate=True, cls_last=True),
    C('fused_fewkeys_ws_exact', [4100], lay=('plain', 2, 2, 200, 32), op='fused', fewkeys_ws=True),
    C('fused_fewkeys_ws_short', [4600], lay=('plain', 2, 2, 200, 32), op='fused', fewkeys_ws=True, ws_short=4),
    # attention dropout on every backward path that takes it (the mask of keep_mult: test_dropout_masks_agree ties it to the kernels)
    C('drop_pair_mfma', [2114, 3114], lay=('plain', 2, 2, 100, 150), op='dqdkv', drop=0.25, mask='min'),
    C('drop_pair_mfma_nt2', [2102, 3102], lay=('plain', 2, 2, 30, 30), op='dqdkv', drop=0.25),
    C('drop_pair_valu', [2500, 3500], lay=('plain', 2, 2, 40, 100), op='dqdkv', ld_pad=4, drop=0.25, o32=True),
    C('drop_split_mfma', [2302, 3302], lay=('plain', 2, 2, 20, 20), op='dqdkv', nsplit=2, drop=0.25),
    C('drop_split_valu_f32', [2600, 3600], lay=('plain', 2, 2, 70, 600), op='dqdkv', nsplit=3, dt='f32', drop=0.25),
    C('drop_fused_fewq', [4200], lay=('plain', 2, 2, 32, 769), op='fused', bwd_ws=True, drop=0.25, o32=True),
]


@gpu
@pytest.mark.parametrize('case', BWD_CASES)
def test_backward_path(ops, case):
    lib = ops.lib
    c = dict(case)
    P, dt, d, (Qp, Kp, Vp, qoff, koff, voff, ooff, ldo), mask, gen = _setup(ops, c)
    H = P.H
    Ldt = ops.L.EGV_F32 if dt == torch.float32 else ops.L.EGV_BF16
    bf = dt == torch.bfloat16
    dO = _fill((P.q_rows, ldo), gen, 1.0, dt)
    # the forward's outputs as the backward reads them: O rounded to the storage type, O32 and lse to fp32, of the fp64 values
    keep = keep_mult(P, d.drop_p, d.drop_seed).cuda() if c.get('drop') else None
    R0 = full_reference(P, Qp, Kp, Vp, qoff, koff, voff, 0.125, mask=mask, keep=keep)
    O = torch.zeros((P.q_rows, ldo), dtype=dt, device='cuda')
    O[:, ooff:ooff + H * HD] = R0['o'][0].reshape(P.q_rows, H * HD).to(dt)
    O32 = None
    if c.get('o32'):
        O32 = torch.zeros((P.q_rows, ldo), dtype=torch.float32, device='cuda')
        O32[:, ooff:ooff + H * HD] = R0['o'][0].reshape(P.q_rows, H * HD).float()
    lse = R0['lse'][0].float().contiguous()
    kinds = {p // 100 for p in c['paths']}
    from32 = O32 is not None or not bf
    R = full_reference(P, Qp, Kp, Vp, qoff, koff, voff, 0.125, mask=mask, dO=dO, ooff=ooff,
                       mfma=bf and not (kinds <= VALU | {0}), o_from32=from32, u_out=U_BF16 if bf else U_F32, keep=keep)
    delta_in = R['delta'][0].float()
    lddq = (3 if P.kind != 'plain' else 1) * H * HD + 8
    lddk = (3 if P.kind != 'plain' else 2) * H * HD + 8
    dQb = Buf(P.q_rows, lddq, dt)
    dKVb = dQb if P.kind != 'plain' else Buf(P.k_rows, lddk, dt)
    dqoff, dkoff, dvoff = 0, (H * HD if P.kind != 'plain' else 0), (2 * H * HD if P.kind != 'plain' else H * HD)
    delta = Buf(P.q_rows, H, torch.float32)
    if P.extra:                  # the CLS query's delta, as its one-query dQ launch leaves it (egv_attn_bwd_dkv reads it)
        cr = P.cls_rows().cuda()
        delta.m[cr] = delta_in[cr]
    d.O, d.dO, d.lse, d.delta = O.data_ptr(), dO.data_ptr(), lse.data_ptr(), delta.ptr()
    d.O32 = O32.data_ptr() if O32 is not None else None
    d.dQ, d.dK, d.dV = dQb.ptr(), dKVb.ptr(), dKVb.ptr()
    d.lddq, d.lddk, d.lddv = lddq, lddk, lddk
    d.dqoff, d.dkoff, d.dvoff = dqoff, dkoff, dvoff
    op = c['op']
    ws = _ws(ops, c, P, d, 1)
    st = ops._st()

    def run():
        paths = []
        if op == 'fused':
            rc = lib.egv_attn_bwd_fused(Ldt, d, st)
            assert rc in (0, 1), rc
            paths.append(ops.attn_last_path())
            if rc == 0:
                return paths
        if op == 'dqdkv' and d.nsplit > 1:
            ws2 = _ws(ops, c, P, d, 1)
            ops.check(lib.egv_attn_bwd_dq(Ldt, d, st), 'egv_attn_bwd_dq')
            paths.append(ops.attn_last_path())
            torch.cuda.synchronize()
            del ws2
            ws3 = _ws(ops, c, P, d, 2)
            ops.check(lib.egv_attn_bwd_dkv(Ldt, d, st), 'egv_attn_bwd_dkv')
            paths.append(ops.attn_last_path())
            torch.cuda.synchronize()
            del ws3
            return paths
        ops.check(lib.egv_attn_bwd_dq(Ldt, d, st), 'egv_attn_bwd_dq')
        paths.append(ops.attn_last_path())
        ops.check(lib.egv_attn_bwd_dkv(Ldt, d, st), 'egv_attn_bwd_dkv')
        paths.append(ops.attn_last_path())
        if op == 'pair':
            assert lib.egv_attn_bwd_pair_covers_extra(Ldt, d) == 1
            ops.check(lib.egv_attn_bwd_extra_reduce(Ldt, d, 1, st), 'egv_attn_bwd_extra_reduce')
            paths.append(ops.attn_last_path())
        return paths

    paths = run()
    torch.cuda.synchronize()
    assert paths == c['paths'], f"ran paths {paths} ({[PATHS.get(p) for p in paths]}), the case says {c['paths']}"
    last = paths[-1] // 100
    cls_owned = P.extra and (last in (43, 45, 47, 51))
    qi, qrows, qlab = _owned_q(P, cls_owned)
    ki = P.kidx()
    krows = torch.cat([ki.reshape(-1), P.cls_rows()]) if cls_owned else ki.reshape(-1)
    klab = P.labels(ki, 'CLS key row' if cls_owned else None)
    W = H * HD
    worst = _check_rows('dQ', dQb.m[:, dqoff:dqoff + W].double().view(P.q_rows, H, HD), R['dq'], qrows, qlab, P, HD)
    worst = max(worst, _check_rows('dK', dKVb.m[:, dkoff:dkoff + W].double().view(P.k_rows, H, HD), R['dk'], krows, klab, P, HD))
    worst = max(worst, _check_rows('dV', dKVb.m[:, dvoff:dvoff + W].double().view(P.k_rows, H, HD), R['dv'], krows, klab, P, HD))
    # delta: the rows the path states it writes (fewkeys / fewq keep it internal, the fused kernels store the group rows)
    drows = qi.reshape(-1)
    if last in (41, 42):
        drows = drows[:0]
    else:
        worst = max(worst, _check_rows('delta', delta.m.double(), R['delta'], drows, P.labels(qi, None), P, 1))
    if P.extra:                  # the CLS rows hold what the test wrote there
        drows = torch.cat([drows, P.cls_rows()])
    assert delta.untouched(drows, 0, H), 'delta: a write outside the rows the path states it writes'
    # canaries: gradient columns / rows nobody owns
    if P.kind == 'plain':
        assert dQb.untouched(qrows, dqoff, dqoff + W), 'dQ: a write outside the owned rows / head columns'
        assert dKVb.untouched(krows, dkoff, dvoff + W), 'dK / dV: a write outside the owned rows / head columns'
    else:
        both = torch.cat([qrows, krows]).unique()
        assert dQb.untouched(both, 0, 3 * W), 'dQKV: a write outside the owned rows / columns'
    first = (dQb.raw.clone(), dKVb.raw.clone())
    run()
    torch.cuda.synchronize()
    assert torch.equal(dQb.raw, first[0]) and torch.equal(dKVb.raw, first[1]), 'two launches differ'
    for p in paths:
        RATIOS[p] = max(RATIOS.get(p, 0.0), worst)


# ---------------------------------------------------------------- dropout masks
def _recover_keep(ops, c):
    """The keep mask a forward path applies, read back through that path: with Q = K = 0 every probability is 1 / nk, and V = the
    identity on a 64-key chunk gives O[q, d] = keep(q, chunk + d) / ((1 - p) nk).  Returns bool [B, 1, H, nq, nk] and the paths run."""
    P, dt, d, (Qp, Kp, Vp, qoff, koff, voff, ooff, ldo), mask, gen = _setup(ops, c)
    assert P.kind == 'plain' and Kp is Vp
    H, nk = P.H, P.nk
    Qp.zero_()
    ws = _ws(ops, c, P, d, 0)
    keep = torch.zeros(P.B, 1, H, P.nq, nk, dtype=torch.bool)
    paths = set()
    for c0 in range(0, nk, HD):
        n = min(HD, nk - c0)
        Kp.zero_()
        v = Kp[:, voff:voff + H * HD].view(P.B, nk, H, HD)
        v[:, c0:c0 + n, :, :n] = torch.eye(n, dtype=dt, device='cuda').view(1, n, 1, n)
        O = torch.zeros(P.q_rows, ldo, dtype=dt, device='cuda')
        lse = torch.zeros(P.q_rows, H, dtype=torch.float32, device='cuda')
        d.O, d.lse = O.data_ptr(), lse.data_ptr()
        ops.check(ops.lib.egv_attn_fwd(ops.L.EGV_F32 if dt == torch.float32 else ops.L.EGV_BF16, d, ops._st()), 'egv_attn_fwd')
        paths.add(ops.attn_last_path())
        torch.cuda.synchronize()
        o = O[:, ooff:ooff + H * HD].view(P.B, P.nq, H, HD).transpose(1, 2)[..., :n]
        keep[:, 0, :, :, c0:c0 + n] = (o != 0).cpu()
    del ws
    return keep, paths


@gpu
@pytest.mark.parametrize('lay,forms', [
    (('plain', 2, 2, 32, 512), [(700, dict(fewq_ws=True)), (918, dict(nsplit=2, mask='zero')), (1000, dict(ld_pad=4)), (1100, dict(nsplit=3, ld_pad=4)),
                                (1100, dict(nsplit=3, dt='f32'))]),
    (('plain', 3, 2, 40, 256), [(518, dict()), (1000, dict(ld_pad=4)), (1000, dict(dt='f32')), (914, dict(nsplit=2))]),
], ids=['fewq_mfmasplit_valu', 'mfma_valu'])
def test_dropout_masks_agree(ops, lay, forms):
    """The keep masks the dropout paths apply for the same (seed, B, H, rows) are identical bit for bit, across the paths and with
    keep_mult, the mask the dropout cases above check against: a forward and a backward on different paths drop the same entries."""
    P = Problem('plain', lay[1], lay[2], nq=lay[3], nk=lay[4])
    want = keep_mult(P, 0.25, 1234) > 0
    for path, f in forms:
        keep, paths = _recover_keep(ops, dict(lay=lay, drop=0.25, seed=1234, **f))
        assert paths == {path}, f'{f}: ran paths {sorted(paths)}, the case says {path}'
        bad = (keep != want).nonzero()
        assert not len(bad), f'path {path} {f}: keep mask differs at (b, g, h, q, k) = {bad[0].tolist()} ({len(bad)} entries)'
    frac = want.double().mean().item()
    assert abs(frac - 0.75) < 0.02, frac


# ---------------------------------------------------------------- refusals
@gpu
@pytest.mark.parametrize('what', ['bad_shape', 'dropout_extra', 'ld_mod4', 'off_mod4', 'split_ws', 'cls_ws', 'fused_ws',
                                  'missing_lse', 'missing_delta', 'missing_dO', 'reduce_no_ws'])
def test_refusals_leave_outputs_alone(ops, what):
    lib = ops.lib
    c = dict(lay=('space', 2, 2, 3, 100) if what in ('dropout_extra', 'cls_ws', 'fused_ws', 'reduce_no_ws') else ('plain', 2, 2, 40, 100),
             separate=what == 'cls_ws')
    P, dt, d, (Qp, Kp, Vp, qoff, koff, voff, ooff, ldo), mask, gen = _setup(ops, c)
    H = P.H
    O = Buf(P.q_rows, ldo, dt)
    lse = Buf(P.q_rows, H, torch.float32)
    delta = Buf(P.q_rows, H, torch.float32)
    dQ = Buf(P.q_rows, 3 * H * HD, dt)
    dO = _fill((P.q_rows, ldo), gen, 1.0, dt)
    d.O, d.lse, d.delta, d.dO = O.ptr(), lse.ptr(), delta.ptr(), dO.data_ptr()
    d.dQ = d.dK = d.dV = dQ.ptr()
    d.lddq = d.lddk = d.lddv = 3 * H * HD
    d.dkoff, d.dvoff = H * HD, 2 * H * HD
    ws = torch.zeros(1 << 16, dtype=torch.float32, device='cuda')
    B = ops.L.EGV_BF16
    entry = lib.egv_attn_fwd
    if what == 'bad_shape':
        d.q_n = 0
    elif what == 'dropout_extra':
        d.drop_p, d.drop_seed = 0.1, 7
    elif what == 'ld_mod4':
        d.ldk = d.ldk - 2
    elif what == 'off_mod4':
        d.voff = d.voff + 2
    elif what == 'split_ws':
        d.nsplit, d.ws, d.ws_bytes = 3, ws.data_ptr(), lib.egv_attn_split_workspace_bytes(0, P.B, P.G, H, P.nq, 3) - 4
    elif what == 'cls_ws':       # separate Q / K / V: the space kernel declines, the MFMA kernel would take the CLS query
        d.ws, d.ws_bytes = ws.data_ptr(), lib.egv_attn_fwd_extra_workspace_bytes(P.B, P.G, H) - 4
    elif what == 'fused_ws':
        entry = lib.egv_attn_bwd_fused
        d.ws, d.ws_bytes = ws.data_ptr(), lib.egv_attn_bwd_fused_workspace_bytes(P.B, P.G, H) - 4
    elif what == 'missing_lse':
        entry, d.lse = lib.egv_attn_bwd_dq, None
    elif what == 'missing_delta':
        entry, d.delta = lib.egv_attn_bwd_dkv, None
    elif what == 'missing_dO':
        entry, d.dO = lib.egv_attn_bwd_fused, None
    elif what == 'reduce_no_ws':
        rc = lib.egv_attn_bwd_extra_reduce(B, d, 1, ops._st())
        entry = None
    if entry is not None:
        rc = entry(B, d, ops._st())
    torch.cuda.synchronize()
    assert rc == -1 and ops.attn_last_path() == 0
    everything = torch.arange(0)
    for buf in (O, lse, delta, dQ):
        assert buf.untouched(everything, 0, 0), 'a refused call wrote an output'


# ---------------------------------------------------------------- coverage of the path table (no GPU)
def test_cases_cover_every_documented_path():
    """Three lists must agree: the kinds the C dispatchers record (every egv_attn_note_path call in csrc/egv_attn*.hip), the kind
    table of this docstring, and the kinds of the paths the cases declare; every code of PATHS has a case and no case names another."""
    import glob
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'egovlpv2_amd', 'csrc')
    in_c = set()
    for f in glob.glob(os.path.join(csrc, 'egv_attn*.hip')):
        for arg in re.findall(r'egv_attn_note_path\(([^;]*)\);', open(f).read()):
            in_c |= {int(x) for x in re.findall(r'\b\d+\b', arg)}
    table = __doc__.split('The kinds:')[1].split('The tile instance')[0]
    documented = {int(x) for x in re.findall(r'(?:^|\s)(\d{1,2})  [A-Za-z<(]', table)}
    assert in_c == documented, ('recorded by the C code, not documented', sorted(in_c - documented),
                                'documented, not recorded', sorted(documented - in_c))
    declared = set()
    for group in (FWD_CASES, BWD_CASES):
        for p in group:
            declared |= set(p.values[0]['paths'])
    declared.discard(0)
    assert {p // 100 for p in declared} == documented, sorted(documented ^ {p // 100 for p in declared})
    assert declared == set(PATHS), (sorted(set(PATHS) - declared), sorted(declared - set(PATHS)))
