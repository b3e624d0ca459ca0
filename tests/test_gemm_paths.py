"""Every kernel path behind the three GEMM entry points -- egv_gemm, egv_gemm_wgrad, egv_gemm_wgrad_grouped -- reached on purpose
and checked element by element against fp64.

Each case names the kernel it must run (the kind code egv_prof_end records, read back through the library's profiler) and the test
asserts it: a dispatch change that moves a shape onto another path fails here until the table is updated.  The kinds:

    0 / 1   generic 128x128 bf16 (NN / b_trans)            7   skinny (<= 16 rows)          12  persistent ping-pong
    4 / 5   generic 128x128 fp32 (NN / b_trans)            8   ring 256x128, or ring wgrad  13  ring 128x128
    2 / 6   generic weight gradient bf16 / fp32             9   small-M weight gradient      14  ping-pong weight gradient
                                                            10  ring weight gradient         15  grouped weight gradient

Paths are reached through shape, stride, pointer alignment and epilogue only (EGV_GEMM_PP / EGV_WGRAD_PP / EGV_WGRAD_SMALL_M are
read once per process and stay at their defaults; EGV_PP_FORCE_BM is read per call).

What every case checks:
  * the reference is fp64 math on the very inputs the kernel saw (already in their storage dtype);
  * element-wise bound |c - ref| <= a |ref| + (1 + a) E, a = the output rounding (2^-8 bf16, 2^-23 fp32) and E the error the fp32
    computation may carry into the rounding: (K + 2) 2^-24 (|A| |B|^T + |bias|) for the accumulation over K (the worst case of
    recursive fp32 summation; bf16 x bf16 products are exact in fp32, fp32 x fp32 ones round once), carried through the epilogue
    with each operation's Lipschitz factor and an fp32 rounding of each epilogue step.  The bf16-mode fast GELU / GELU' forms
    (gelu_fast_f, dgelu_fast_f in egv_common.h) add their documented maximum error: x Phi(x) within 4.0e-5 relative / 6.6e-6
    absolute, the derivative within 1.8e-5 absolute; the fp32 forms (libm erff / tanhf / __expf) a few ulps, taken as
    2^-19 (1 + |x|);
  * the worst element is reported per region (body, last row tile, last column tile, corner) so a miss names its region;
  * outputs live inside canary buffers (leading dimension above N, guard rows after the last row, guard elements in front) filled
    with a NaN bit pattern that must come back bit-identical.
"""
import math
import zlib

import pytest
import torch

gpu = pytest.mark.gpu

U_BF16 = 2.0 ** -8          # unit roundoff of the bf16 output
U_F32 = 2.0 ** -23          # (about) the fp32 output rounding
U_ACC = 2.0 ** -24          # fp32 accumulation / epilogue arithmetic
GELU_FAST_REL, GELU_FAST_ABS, DGELU_FAST_ABS = 4.0e-5, 6.6e-6, 1.8e-5     # egv_common.h: documented error of the bf16-mode forms
LIBM = 2.0 ** -19           # fp32-mode erff / tanhf / __expf: a few ulps of the argument's scale
GELU_LIP = 1.13             # max |gelu'| (1.1289 at x = 2.4)
CANARY = {torch.bfloat16: (torch.int16, 0x7FA5), torch.float32: (torch.int32, 0x7FA5A5A5)}   # quiet NaNs nothing computes
TILE = (128, 128)


# ---------------------------------------------------------------- checker (pure torch: runs on the CPU too)
def region_report(out, ref, bound, row_ids=None, M=None, tile=TILE):
    """Worst |out - ref| / bound per region of the [M, N] output: 'body', 'last row tile', 'last column tile', 'corner'.
    row_ids: global row of each row of out / ref when only sampled rows are compared (M: the full row count).
    Returns {region: (ratio, row, col, out, ref, bound)}; NaN / inf in out count as an infinite ratio."""
    out, ref, bound = out.double(), ref.double(), bound.double()
    rows, N = ref.shape
    if row_ids is None:
        row_ids, M = torch.arange(rows, device=ref.device), rows
    row_ids = row_ids.to(ref.device)
    err = (out - ref).abs()
    ratio = torch.where(err <= bound, err / bound.clamp_min(1e-300), torch.full_like(err, math.inf))
    ratio = torch.where(err == 0, torch.zeros_like(err), ratio)
    r0, c0 = ((M - 1) // tile[0]) * tile[0], ((N - 1) // tile[1]) * tile[1]
    in_last_row = (row_ids >= r0)[:, None]
    in_last_col = (torch.arange(N, device=ref.device) >= c0)[None, :]
    masks = {'body': ~in_last_row & ~in_last_col, 'last row tile': in_last_row & ~in_last_col,
             'last column tile': ~in_last_row & in_last_col, 'corner': in_last_row & in_last_col}
    rep = {}
    for name, m in masks.items():
        m = m.expand(rows, N)
        if not bool(m.any()):
            continue
        r = torch.where(m, ratio, torch.full_like(ratio, -1.0))
        i = int(torch.argmax(r))
        ri, ci = i // N, i % N
        rep[name] = (float(r.view(-1)[i]), int(row_ids[ri]), ci, float(out[ri, ci]), float(ref[ri, ci]), float(bound[ri, ci]))
    return rep


def assert_within(what, out, ref, bound, **kw):
    rep = region_report(out, ref, bound, **kw)
    bad = {k: v for k, v in rep.items() if not v[0] <= 1.0}
    assert not bad, what + ': ' + '; '.join(f"{k}: worst at ({v[1]}, {v[2]}) got {v[3]!r} want {v[4]!r} (bound {v[5]:.3g}, {v[0]:.3g}x)"
                                            for k, v in bad.items())
    return rep


def gelu64(x):
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2)))


def dgelu64(x):
    return 0.5 * (1 + torch.erf(x / math.sqrt(2))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


def gemm_reference(A, Bm, *, bf16, bias=None, act=0, gate=None, res1=None, res2=None, aux=None, dact=0, scale=1.0, want_pre=False):
    """fp64 epilogue(scale * A @ Bm^T) of egv_gemm and its element-wise error bound.  A [M, K], Bm [N, K] as the kernel reads them
    (Aop / Bop); every operand already in fp64.  Returns (out, bound, pre, pre_bound)."""
    K = A.shape[1]
    z = (A @ Bm.t()) * scale
    S = (A.abs() @ Bm.abs().t()) * abs(scale)
    if bias is not None:
        z = z + bias
        S = S + bias.abs()
    E = (K + 2) * U_ACC * S + 4 * U_ACC * z.abs()                      # accumulation; scale and bias roundings
    a = U_BF16 if bf16 else U_F32
    pre = pre_b = None
    if want_pre:
        if act == 4:                                                   # EGV_ACT_GELU_D: the saved tensor is gelu'(z)
            pre = dgelu64(z)
            pre_b = a * pre.abs() + (1 + a) * (E + (DGELU_FAST_ABS if bf16 else LIBM * (1 + z.abs())))
        else:
            pre, pre_b = z, a * z.abs() + (1 + a) * E
    y = z
    if act in (1, 4):
        y = gelu64(z)
        E = GELU_LIP * E + ((GELU_FAST_REL * y.abs() + GELU_FAST_ABS) if bf16 else LIBM * (1 + z.abs()))
    elif act == 2:
        y = torch.relu(z)
    elif act == 3:
        y = torch.tanh(z)
        E = E + LIBM * (1 + z.abs())
    if gate is not None:
        y = y * gate
        E = E * abs(gate) + U_ACC * y.abs()
    for r in (res1, res2):
        if r is not None:
            y = y + r
            E = E + 2 * U_ACC * (y.abs() + r.abs())
    if dact:
        if dact == 1:
            d, dd = dgelu64(aux), (DGELU_FAST_ABS if bf16 else LIBM * (1 + aux.abs()))
        elif dact == 2:
            d, dd = (aux > 0).double(), 0.0
        else:
            d, dd = 1 - aux * aux, 4 * U_ACC * (1 + aux * aux)
        E = E * d.abs() + y.abs() * dd + U_ACC * (y * d).abs()
        y = y * d
    return y, a * y.abs() + (1 + a) * E, pre, pre_b


def wgrad_reference(dY, X, sc, fp32_inputs=False):
    """fp64 dW = sc * dY^T X, db = sc * colsum(dY) and their bounds (fp32 outputs; the reduction over the M rows, split or not)."""
    M = dY.shape[0]
    dw = (dY.t() @ X) * sc
    db = dY.sum(0) * sc
    b = (M + 66 + (1 if fp32_inputs else 0)) * U_ACC                   # M-term sum plus up to 64 slab partial sums
    dwb = U_F32 * dw.abs() + b * (dY.abs().t() @ X.abs()) * abs(sc) + 4 * U_ACC * dw.abs()
    dbb = U_F32 * db.abs() + b * dY.abs().sum(0) * abs(sc) + 4 * U_ACC * db.abs()
    return dw, dwb, db, dbb


def bf16_ulp(x):
    """one bf16 ulp at the magnitude of x (fp64 tensor)"""
    e = torch.floor(torch.log2(x.abs().clamp_min(1e-30)))
    return torch.pow(2.0, e - 7)


# ---------------------------------------------------------------- self-test of the checker (no GPU)
def test_checker_rejects_one_ulp_in_ragged_tile_and_a_dropped_row():
    """The bound must not pass anything: an exactly rounded bf16 result passes; moving one element of the ragged corner tile by one bf16
    ulp of its magnitude fails and names the corner; a product computed without the last row of A fails in the last row tile."""
    g = torch.Generator().manual_seed(5)
    M, N, K = 200, 136, 64
    A = torch.randn(M, K, generator=g).to(torch.bfloat16).double()
    Bm = (torch.randn(N, K, generator=g) / 8).to(torch.bfloat16).double()
    bias = torch.randn(N, generator=g).float().double()
    ref, bound, _, _ = gemm_reference(A, Bm, bf16=True, bias=bias)
    good = ref.to(torch.bfloat16)
    assert_within('exact rounding', good, ref, bound)
    # an element of the corner tile (rows >= 128, cols >= 128) well inside its binade, moved one ulp away from ref
    cand = [(m, n) for m in range(128, M) for n in range(128, N)
            if abs(ref[m, n]) > 0.5 and float(ref[m, n].abs() / bf16_ulp(ref[m, n].abs())) < 192]
    m, n = cand[0]
    bad = good.double().clone()
    step = float(bf16_ulp(ref[m, n].abs()))
    bad[m, n] = bad[m, n] + (step if bad[m, n] >= ref[m, n] else -step)
    rep = region_report(bad, ref, bound)
    assert rep['corner'][0] > 1.0 and rep['corner'][1:3] == (m, n)
    assert all(v[0] <= 1.0 for k, v in rep.items() if k != 'corner')
    with pytest.raises(AssertionError, match='corner'):
        assert_within('one ulp', bad, ref, bound)
    dropped = torch.cat([A[:-1] @ Bm.t() + bias, torch.zeros(1, N, dtype=torch.float64)]).to(torch.bfloat16)
    with pytest.raises(AssertionError, match='last row tile'):
        assert_within('dropped row', dropped, ref, bound)
    # the weight gradient's bound: dW without the last token row of dY / X fails (the fp32 output has a much tighter rounding term)
    dY = torch.randn(300, 136, generator=g).to(torch.bfloat16).double()
    X = torch.randn(300, 72, generator=g).to(torch.bfloat16).double()
    dw, dwb, db, dbb = wgrad_reference(dY, X, 1.0)
    assert_within('exact dW', dw.float(), dw, dwb)
    with pytest.raises(AssertionError):
        assert_within('dW without a token', (dY[:-1].t() @ X[:-1]).float(), dw, dwb)
    with pytest.raises(AssertionError):
        assert_within('db without a token', dY[:-1].sum(0, keepdim=True).float(), db[None], dbb[None])


# ---------------------------------------------------------------- GPU harness
@pytest.fixture(scope='module')
def ops():
    from egovlpv2_amd import hipops
    return hipops


def kinds_of(ops, fn):
    """Run fn with the library's profiler on; return (the kind codes the call recorded, fn's result)."""
    ops.prof_enable(True)
    try:
        ops.prof_reset()
        r = fn()
        recs = ops.prof_collect()
    finally:
        ops.prof_enable(False)
    return [rec[2] for rec in recs], r


class Canaried:
    """A [rows, cols] matrix at row pitch ld inside a buffer filled with a NaN bit pattern: `off` elements in front of it, `guard`
    rows behind it, the columns cols..ld-1 of every row.  untouched() is True if every element outside the matrix kept its bits."""

    def __init__(self, rows, cols, ld, dtype, off=0, guard=3, device='cuda'):
        itype, pat = CANARY[dtype]
        n = off + (rows + guard) * ld
        self.raw = torch.full((n,), pat, dtype=itype, device=device)
        self.pat = pat
        self.m = self.raw.view(dtype)[off:off + rows * ld].view(rows, ld)[:, :cols]
        self.outside = torch.ones(n, dtype=torch.bool, device=device)
        self.outside[off:off + rows * ld].view(rows, ld)[:, :cols] = False

    def ptr(self):
        return self.m.data_ptr()

    def untouched(self):
        return bool((self.raw[self.outside] == self.pat).all())


def _rand(shape, dtype, scale, gen, device='cuda'):
    return (torch.randn(shape, generator=gen, device=device) * scale).to(dtype)


def G(name, kind, M, N, K, **kw):
    return pytest.param(dict(kind=kind, M=M, N=N, K=K, **kw), id=name)


M2, N2 = 2056, 2048        # 9 x 8 = 72 tiles of 256^2 (>= 64: the persistent kernel is tried); 9 x 16 = 144 of 256x128 (> 128)
# Expected kinds follow the gates of egv_gemm (csrc/egv_gemm.hip), egv_gemm2_launch (csrc/egv_gemm2.hip) and egv_gemm3_launch
# (csrc/egv_gemm3.hip).  bf16 unless dt='f32'.  off: element offsets of operands from a 16-byte-aligned address.
GEMM_CASES = [
    # skinny: bf16 NN, M <= 16, N >= 512, K >= 512, K % 8 == 0, act in {0..3}, pre only with GELU at ldr == ldc, nothing else
    G('skinny_m1', 7, 1, 512, 512),
    G('skinny_m16_k520_relu_bias', 7, 16, 512, 520, act=2, bias=True),
    G('skinny_n520_tanh_ldc', 7, 16, 520, 512, act=3, ldc=528),
    G('skinny_gelu_pre', 7, 5, 1024, 512, act=1, pre=True, bias=True),
    G('skinny_leaves_m17', 0, 17, 512, 512),
    G('skinny_leaves_n504', 0, 16, 504, 512),
    G('skinny_leaves_k516', 0, 8, 512, 516),
    G('skinny_leaves_gate', 0, 4, 512, 512, gate=0.75),
    G('skinny_leaves_res1', 0, 4, 512, 512, res1=True),
    G('skinny_leaves_scale', 0, 4, 512, 512, scale=0.5),
    G('skinny_leaves_pre_ldr', 0, 4, 512, 512, act=1, pre=True, ldr=520),
    # ring 128x128: M >= 128, K % 64, N % 8, ldc % 8, ldr % 8, 16-byte operands; fewer than 64 tiles of 256^2 and <= 128 of 256x128
    G('ring128_bias', 13, 129, 264, 192, bias=True),
    G('ring128_gelu_pre', 13, 200, 256, 128, act=1, pre=True, bias=True),
    G('ring128_geluD_pre', 13, 200, 256, 128, act=4, pre=True, bias=True),
    G('ring128_res_gate', 13, 200, 256, 128, res1=True, res2=True, gate=0.6, bias=True),
    G('ring128_dact', 13, 136, 320, 192, dact=1),
    G('ring128_relu_scale', 13, 256, 128, 256, act=2, scale=0.5),
    G('ring128_ldr_ne_ldc', 13, 200, 256, 128, res1=True, pre=True, act=1, ldc=264, ldr=272),
    G('ring128_lda_ldb', 13, 200, 264, 192, lda=200, ldb=208),
    G('ring_leaves_m127', 0, 127, 264, 192),
    G('ring_leaves_n_mod8', 0, 200, 260, 192),
    G('ring_leaves_k_mod64', 0, 200, 264, 160),
    G('ring_leaves_ldc_mod8', 0, 200, 264, 192, ldc=268),
    G('ring_leaves_c_off1', 0, 200, 264, 192, off={'C': 1}),
    # ring 256x128: > 128 tiles of 256x128 while the persistent kernel declines the call
    G('ring256_relu_bias', 8, M2, N2, 192, act=2, bias=True),
    G('ring256_tanh', 8, M2, N2, 192, act=3),
    G('ring256_scale', 8, M2, N2, 192, scale=0.5),
    G('ring256_res1_k1472', 8, M2, N2, 1472, res1=True),            # 256-row tiles: res1 needs K >= EGV_PP_RES_MINK (1536)
    G('ring256_k128', 8, M2, N2, 128),                             # persistent: K >= 192
    G('ring256_dact_bias', 8, M2, N2, 192, dact=1, bias=True),     # persistent: GELU' without bias only
    G('ring256_res1_bm192_k704', 8, M2, N2, 704, res1=True, bm=192),   # 192-row tiles: res1 needs K >= 768
    G('ring256_gated2_k704', 8, M2, N2, 704, res1=True, res2=True, gate=0.6),
    # persistent ping-pong: >= 64 tiles of 256^2, K % 64, K >= 192, N % 64, scale 1, its epilogue kinds
    G('pp_plain', 12, M2, N2, 192),
    G('pp_bias_k768', 12, M2, N2, 768, bias=True),
    G('pp_n1984_bias', 12, M2, 1984, 192, bias=True),
    G('pp_gelu', 12, M2, N2, 192, act=1, bias=True),
    G('pp_gelu_pre', 12, M2, N2, 192, act=1, pre=True, bias=True),
    G('pp_geluD_pre', 12, M2, N2, 192, act=4, pre=True, bias=True),
    G('pp_dact', 12, M2, N2, 192, dact=1),
    G('pp_gate', 12, M2, N2, 192, gate=0.6),
    G('pp_res1_k1536', 12, M2, N2, 1536, res1=True),
    G('pp_res1_bm192_k768', 12, M2, N2, 768, res1=True, bm=192),
    G('pp_gated2', 12, M2, N2, 768, res1=True, res2=True, gate=0.6),
    G('pp_gated2_pre', 12, M2, N2, 768, res1=True, res2=True, gate=0.6, pre=True),
    G('pp_bm256', 12, M2, N2, 192, bm=256),
    G('pp_bm224', 12, M2, N2, 192, bm=224),
    G('pp_bm192', 12, M2, N2, 192, bm=192),
    G('pp_bm160', 12, M2, N2, 192, bm=160),
    G('pp_bm128', 12, M2, N2, 192, bm=128),
    G('pp_bias_bm160', 12, M2, N2, 192, bias=True, bm=160),
    G('pp_gelu_pre_bm192', 12, M2, N2, 192, act=1, pre=True, bm=192),   # GELU kinds are built for 256 rows: the forced height is ignored
    # generic 128x128, fp32 (kind 4 NN, 5 b_trans): every epilogue
    *[G(f'gen_f32_{f}_{e}', 4 + bt, 300, 200, 100, dt='f32', bt=bt, **kw)
      for bt, f in ((0, 'nn'), (1, 'nt'))
      for e, kw in (('bias_gelu_pre', dict(bias=True, act=1, pre=True)), ('relu_gate', dict(act=2, gate=0.7)),
                    ('tanh_res2_scale', dict(act=3, res1=True, res2=True, scale=0.5)), ('dgelu_bias', dict(dact=1, bias=True)),
                    ('drelu', dict(dact=2)), ('dtanh_scale_gate', dict(dact=3, scale=1.5, gate=0.8)))],
    G('gen_f32_tt_bias', 5, 136, 200, 96, dt='f32', at=1, bt=1, bias=True),
    G('gen_f32_lda_ldb', 4, 300, 200, 100, dt='f32', lda=103, ldb=101, bias=True),
    G('gen_bf16_tt', 1, 136, 200, 96, at=1, bt=1),
    G('gen_bf16_tt_out_f32_k250', 1, 136, 200, 250, at=1, bt=1, of32=1, bias=True),
    G('ringwg_bf16_tt_out_f32', 8, 136, 200, 256, at=1, bt=1, of32=1, bias=True),
    G('gen_bf16_nt_dgelu', 1, 300, 200, 256, bt=1, dact=1),
    G('gen_bf16_nt_lda_ldb', 1, 100, 200, 96, bt=1, lda=104, ldb=208),
    G('gen_bf16_ldr4', 0, 100, 200, 96, act=1, pre=True, res1=True, res2=True, ldc=208, ldr=204),
    G('gen_bf16_ldr_odd', 0, 100, 200, 96, act=1, pre=True, res1=True, res2=True, ldc=208, ldr=202),
    G('gen_bf16_dact_ldr', 0, 100, 200, 96, dact=3, ldr=206),
    # misaligned epilogue operands: no wide access through them (C: the control, gated by c_vec_ok before)
    *[G(f'misal_gen_{w}{o}', 0, 100, 200, 96, off={w: o}, **kw)
      for w, o, kw in (('res1', 1, dict(res1=True, res2=True, act=1, pre=True)), ('res2', 2, dict(res1=True, res2=True, act=1, pre=True)),
                       ('pre', 3, dict(res1=True, res2=True, act=1, pre=True)), ('aux', 1, dict(dact=1)), ('C', 1, dict(res1=True)))],
    G('misal_gen_f32_res1_1', 4, 300, 200, 100, dt='f32', res1=True, res2=True, act=4, pre=True, off={'res1': 1}),
    G('misal_gen_f32_aux_2', 5, 300, 200, 100, dt='f32', bt=1, dact=1, off={'aux': 2}),
    *[G(f'misal_ring_{w}{o}', 0, 200, 264, 192, off={w: o}, **kw)
      for w, o, kw in (('res1', 1, dict(res1=True)), ('res2', 2, dict(res1=True, res2=True, gate=0.6)), ('pre', 3, dict(act=1, pre=True)),
                       ('aux', 1, dict(dact=1)), ('C', 1, dict(res1=True)))],
    *[G(f'misal_pp_{w}{o}', 0, M2, N2, 768, off={w: o}, **kw)
      for w, o, kw in (('res2', 1, dict(res1=True, res2=True, gate=0.6)), ('res1', 1, dict(res1=True, res2=True, gate=0.6)),
                       ('pre', 2, dict(act=1, pre=True)), ('aux', 3, dict(dact=1)), ('C', 1, dict(bias=True)))],
    G('pp_gated2_res2_off8', 12, M2, N2, 768, res1=True, res2=True, gate=0.6, off={'res2': 8}),   # 16 bytes: still aligned
]


@gpu
@pytest.mark.parametrize('case', GEMM_CASES)
def test_gemm_path(ops, case, monkeypatch):
    L, lib = ops.L, ops.lib
    c = dict(case)
    M, N, K = c['M'], c['N'], c['K']
    f32 = c.get('dt') == 'f32'
    dt = torch.float32 if f32 else torch.bfloat16
    at, bt, of32 = c.get('at', 0), c.get('bt', 0), c.get('of32', 0)
    act, dact, scale, gate_v = c.get('act', 0), c.get('dact', 0), c.get('scale', 1.0), c.get('gate')
    off = c.get('off', {})
    ldc = c.get('ldc', N)
    ldr = c.get('ldr', ldc)
    odt = torch.float32 if (of32 or f32) else torch.bfloat16
    gen = torch.Generator(device='cuda').manual_seed(zlib.crc32(repr(sorted(c.items())).encode()))
    # operands as stored: A [M, lda] or [K, lda >= M]; B [N, ldb] or [K, ldb >= N]
    a_rows, a_cols = (K, M) if at else (M, K)
    b_rows, b_cols = (K, N) if bt else (N, K)
    lda, ldb = c.get('lda', a_cols), c.get('ldb', b_cols)
    A = Canaried(a_rows, a_cols, lda, dt, off.get('A', 0), guard=1)
    Bw = Canaried(b_rows, b_cols, ldb, dt, off.get('B', 0), guard=1)
    A.m.copy_(_rand((a_rows, a_cols), dt, 1.0, gen))
    Bw.m.copy_(_rand((b_rows, b_cols), dt, 1.0 / math.sqrt(K), gen))
    Cb = Canaried(M, N, ldc, odt, off.get('C', 0))
    bias = _rand((N,), torch.float32, 0.5, gen) if c.get('bias') else None
    gate = torch.tensor([gate_v], dtype=torch.float32, device='cuda') if gate_v is not None else None
    ep = {}
    for w in ('res1', 'res2', 'pre', 'aux'):
        if c.get(w) or (w == 'aux' and dact):
            ep[w] = Canaried(M, N, ldr, dt, off.get(w, 0))
    for w in ('res1', 'res2'):
        if w in ep:
            ep[w].m.copy_(_rand((M, N), dt, 1.0, gen))
    if 'aux' in ep:
        ep['aux'].m.copy_(_rand((M, N), dt, 1.0, gen) if dact != 3 else (torch.rand((M, N), generator=gen, device='cuda') * 1.8 - 0.9).to(dt))
    p = lambda w: ep[w].ptr() if w in ep else None          # noqa: E731
    if 'bm' in c:
        monkeypatch.setenv('EGV_PP_FORCE_BM', str(c['bm']))
    kinds, rc = kinds_of(ops, lambda: lib.egv_gemm(L.EGV_F32 if f32 else L.EGV_BF16, at, bt, M, N, K, A.ptr(), lda, Bw.ptr(), ldb, Cb.ptr(), ldc,
                                                    of32, ops._p(bias), act, ops._p(gate), p('res1'), p('res2'), p('pre'), p('aux'), dact,
                                                    c.get('ldr', 0), float(scale), ops._st()))
    monkeypatch.delenv('EGV_PP_FORCE_BM', raising=False)
    ops.check(rc, 'egv_gemm')
    torch.cuda.synchronize()
    assert kinds == [c['kind']], f"ran kind {kinds}, the table says {c['kind']}"
    d = lambda t: None if t is None else t.double()          # noqa: E731
    Aop = A.m.double().t() if at else A.m.double()
    Bop = Bw.m.double().t() if bt else Bw.m.double()
    ref, bound, pre_ref, pre_b = gemm_reference(Aop, Bop, bf16=not f32, bias=d(bias), act=act, gate=gate_v,
                                                res1=d(ep['res1'].m) if 'res1' in ep else None, res2=d(ep['res2'].m) if 'res2' in ep else None,
                                                aux=d(ep['aux'].m) if 'aux' in ep else None, dact=dact, scale=scale, want_pre='pre' in ep)
    if of32 and not f32:           # fp32 output of a bf16 GEMM: the output rounding is fp32's
        bound = bound - U_BF16 * ref.abs() + U_F32 * ref.abs()
    assert_within('C', Cb.m, ref, bound)
    assert Cb.untouched(), 'C: a write outside [M, N] (padding columns, guard rows or the elements in front)'
    if 'pre' in ep:
        assert_within('pre', ep['pre'].m, pre_ref, pre_b)
        assert ep['pre'].untouched(), 'pre: a write outside [M, N]'
    for w in ('res1', 'res2', 'aux'):
        if w in ep:
            assert ep[w].untouched(), f'{w}: the read-only operand buffer changed'


# ---------------------------------------------------------------- egv_gemm_wgrad: dW[N, K] = scale * gate * dY^T X, db[N]
def W(name, kind, M, N, K, **kw):
    return pytest.param(dict(kind=kind, M=M, N=N, K=K, **kw), id=name)


# Expected kinds follow egv_gemm_wgrad (csrc/egv_gemm.hip), egv_gemm2_launch's a_trans branch and egv_gemm4_launch.
WGRAD_CASES = [
    # small-M outer product: bf16, M <= 16, K % 4, ldx % 4, X 8-byte and dW 16-byte aligned
    W('smallm_m1_bias', 9, 1, 300, 256, bias=True),
    W('smallm_m16_scale_gate', 9, 16, 300, 256, bias=True, scale=0.5, gate=0.8),
    W('smallm_strides', 9, 8, 300, 256, ldy=304, ldx=260, bias=True),
    W('smallm_leaves_m17', 2, 17, 300, 256, bias=True),                        # generic + egv_colsum for db
    W('smallm_leaves_k258', 2, 8, 300, 258),
    W('smallm_leaves_ldx', 2, 8, 300, 256, ldx=258),
    # ring weight gradient: bf16, N >= 128, K >= 64, M >= 256, N % 8, K % 8
    W('ring_bias_direct', 10, 300, 136, 200, bias=True),                       # one split, no scale / gate: db from the kernel's sums
    W('ring_splits_scale_gate', 10, 2048, 256, 256, bias=True, scale=0.5, gate=0.8),   # 4 splits: fused bias reduce, scaled + gated
    W('ring_strides', 10, 1100, 264, 192, bias=True, ldy=272, ldx=200),
    W('ring_leaves_n140', 2, 300, 140, 200, bias=True),                        # generic + egv_colsum
    W('ring_leaves_k204', 2, 300, 136, 204, bias=True, scale=2.0),
    W('ring_leaves_m255', 2, 255, 136, 200),
    # ping-pong weight gradient: bf16, N and K multiples of 256, M >= 4096, (N / 256) (K / 256) <= 128
    W('pp_m4096', 14, 4096, 256, 512, bias=True, gate=0.8),
    W('pp_m4104', 14, 4104, 512, 256, bias=True),
    W('pp_leaves_m4095', 10, 4095, 256, 512, bias=True),
    W('pp_leaves_n776', 10, 4096, 776, 512),
    W('pp_128_tiles', 14, 4096, 2048, 4096, bias=True, rows=True),
    W('pp_leaves_135_tiles', 10, 4096, 2304, 3840, rows=True),
    # fp32: the generic kernel, split over M when M allows, db through egv_colsum
    W('f32_m8', 6, 8, 100, 64, dt='f32', bias=True),
    W('f32_m1024_splits', 6, 1024, 200, 136, dt='f32', bias=True, scale=0.5, gate=0.8),
    W('f32_m4099_splits', 6, 4099, 130, 72, dt='f32', bias=True, ldy=136, ldx=76),
]


@gpu
@pytest.mark.parametrize('case', WGRAD_CASES)
def test_wgrad_path(ops, case):
    L, lib = ops.L, ops.lib
    c = dict(case)
    M, N, K = c['M'], c['N'], c['K']
    f32 = c.get('dt') == 'f32'
    dt = torch.float32 if f32 else torch.bfloat16
    ldy, ldx = c.get('ldy', N), c.get('ldx', K)
    scale, gate_v = c.get('scale', 1.0), c.get('gate')
    gen = torch.Generator(device='cuda').manual_seed(M * 7919 + N * 31 + K)
    dY = Canaried(M, N, ldy, dt, guard=1)
    X = Canaried(M, K, ldx, dt, guard=1)
    dY.m.copy_(_rand((M, N), dt, 1.0, gen))
    X.m.copy_(_rand((M, K), dt, 1.0, gen))
    dW = Canaried(N, K, K, torch.float32, off=4, guard=2)                   # dW has row pitch K: canaries in front and behind
    db = Canaried(1, N, N, torch.float32, off=4, guard=1) if c.get('bias') else None
    gate = torch.tensor([gate_v], dtype=torch.float32, device='cuda') if gate_v is not None else None
    nb = lib.egv_gemm_wgrad_workspace_bytes(N, K, M)
    ws = torch.empty(nb, dtype=torch.uint8, device='cuda')
    kinds, rc = kinds_of(ops, lambda: lib.egv_gemm_wgrad(L.EGV_F32 if f32 else L.EGV_BF16, M, N, K, dY.ptr(), ldy, X.ptr(), ldx, dW.ptr(),
                                                          db.ptr() if db is not None else None, float(scale), ops._p(gate), ws.data_ptr(),
                                                          nb, ops._st()))
    ops.check(rc, 'egv_gemm_wgrad')
    torch.cuda.synchronize()
    assert kinds == [c['kind']], f"ran kind {kinds}, the table says {c['kind']}"
    sc = scale * (gate_v if gate_v is not None else 1.0)
    Y64, X64 = dY.m.double(), X.m.double()
    rows = None
    if c.get('rows'):              # big outputs: the first and the last 256-row tile of dW and a stripe in between
        rows = torch.cat([torch.arange(0, 8), torch.arange(N // 2 - 3, N // 2 + 5), torch.arange(N - 256, N)]).cuda()
        Y64 = Y64[:, rows]
    ref, refb, dbr, dbb = wgrad_reference(Y64, X64, sc, fp32_inputs=f32)
    got = dW.m if rows is None else dW.m[rows]
    assert_within('dW', got, ref, refb, row_ids=rows, M=N, tile=(256, 256))
    assert dW.untouched(), 'dW: a write outside [N, K]'
    if db is not None:
        assert_within('db', db.m if rows is None else db.m[:, rows], dbr[None], dbb[None])
        assert db.untouched(), 'db: a write outside [N]'
    assert dY.untouched() and X.untouched()


# ---------------------------------------------------------------- egv_gemm_wgrad_grouped
def _prob_array(L, probs):
    arr = (L.WgradProblem * len(probs))()
    for i, q in enumerate(probs):
        arr[i].dy, arr[i].ldy, arr[i].x, arr[i].ldx = q['dy'].ptr(), q['ldy'], q['x'].ptr(), q['ldx']
        arr[i].dw, arr[i].db = q['dw'].ptr(), (q['db'].ptr() if q['db'] is not None else None)
        arr[i].gate, arr[i].N, arr[i].K, arr[i].accumulate = (q['gate'].data_ptr() if q['gate'] is not None else None), q['N'], q['K'], q.get('acc', 0)
    return arr


def _make_group(M, shapes, gen, pad=False):
    """shapes: [(N, K, gated, bias)]; operands with padded leading dimensions when pad (multiples of 8 above N / K)"""
    probs = []
    for i, (N, K, gated, bias) in enumerate(shapes):
        ldy, ldx = (N + 8 * (i % 3 + 1), K + 16) if pad else (N, K)
        q = dict(N=N, K=K, ldy=ldy, ldx=ldx, dy=Canaried(M, N, ldy, torch.bfloat16, guard=1), x=Canaried(M, K, ldx, torch.bfloat16, guard=1),
                 gate=torch.tensor([0.5 + 0.1 * i], dtype=torch.float32, device='cuda') if gated else None)
        q['dy'].m.copy_(_rand((M, N), torch.bfloat16, 1.0, gen))
        q['x'].m.copy_(_rand((M, K), torch.bfloat16, 1.0, gen))
        q['dw'] = Canaried(N, K, K, torch.float32, off=4, guard=1)
        q['db'] = Canaried(1, N, N, torch.float32, off=4, guard=1) if bias else None
        probs.append(q)
    return probs


def _grouped(ops, M, probs, cus):
    L, lib = ops.L, ops.lib
    arr = _prob_array(L, probs)
    nb = lib.egv_gemm_wgrad_grouped_workspace_bytes(M, len(probs), arr, cus)
    if nb < 0:
        return None, nb
    ws = torch.empty(max(nb, 16), dtype=torch.uint8, device='cuda')
    kinds, rc = kinds_of(ops, lambda: lib.egv_gemm_wgrad_grouped(L.EGV_BF16, M, len(probs), arr, cus, ws.data_ptr(), nb, ops._st()))
    ops.check(rc, 'egv_gemm_wgrad_grouped')
    torch.cuda.synchronize()
    return kinds, nb


ONE = [(256, 256, False, True)]
D768 = [(2304, 768, False, True), (768, 768, False, True), (3072, 768, False, True), (768, 3072, False, True),
        (768, 768, True, True), (768, 768, True, False)]      # qkv, proj, fc1, fc2, a gated proj (i2t) and a gated one without bias


@gpu
@pytest.mark.parametrize('M,shapes,pad', [(M, s, pad) for M in (64, 100, 1100, 4104) for s in (ONE, D768) for pad in (False, True)
                                          if not (pad and s is ONE and M in (64, 1100))],
                         ids=lambda v: {id(ONE): 'one_256', id(D768): 'd768_block'}.get(id(v), str(v)))
def test_grouped_plans_against_fp64(ops, M, shapes, pad):
    """Every CU grant's plan (24, 96, all CUs; one, several or no reduction splits, several phases on small grants) against fp64, twice
    bit for bit, every dW / db inside its canaries.  Padded operand pitches (multiples of 8 above N / K) on part of the calls."""
    gen = torch.Generator(device='cuda').manual_seed(M + 17 * len(shapes) + pad)
    probs = _make_group(M, shapes, gen, pad)
    refs = []
    for q in probs:
        sc = float(q['gate']) if q['gate'] is not None else 1.0
        refs.append(wgrad_reference(q['dy'].m.double(), q['x'].m.double(), sc))
    planned = 0
    for cus in (24, 96, 0):
        kinds, nb = _grouped(ops, M, probs, cus)
        if kinds is None:
            continue
        planned += 1
        assert kinds == [15]
        first = [(q['dw'].m.clone(), q['db'].m.clone() if q['db'] is not None else None) for q in probs]
        for i, (q, (dw, dwb, db, dbb)) in enumerate(zip(probs, refs)):
            assert_within(f'cus={cus} problem {i} dW', q['dw'].m, dw, dwb, tile=(256, 256))
            assert q['dw'].untouched(), f'cus={cus} problem {i}: a write outside dW'
            if q['db'] is not None:
                assert_within(f'cus={cus} problem {i} db', q['db'].m, db[None], dbb[None], tile=(1, 256))
                assert q['db'].untouched(), f'cus={cus} problem {i}: a write outside db'
        _grouped(ops, M, probs, cus)
        for i, (q, (dw0, db0)) in enumerate(zip(probs, first)):
            assert torch.equal(q['dw'].m, dw0), f'cus={cus} problem {i}: dW differs between two launches'
            if db0 is not None:
                assert torch.equal(q['db'].m, db0), f'cus={cus} problem {i}: db differs between two launches'
    assert planned == 3, 'every grant of 24 CUs or more has a plan for these groups'


@gpu
@pytest.mark.parametrize('M,cus', [(64, 0), (4104, 0), (1100, 24)], ids=['no_splits', 'splits', 'phases'])
def test_grouped_accumulate_is_a_separate_fp32_add(ops, M, cus):
    """accumulate = 1 (beta = 1) writes prefill + (the same problem with accumulate = 0): the bits of a torch fp32 add."""
    gen = torch.Generator(device='cuda').manual_seed(M + cus)
    shapes = ONE if cus == 0 else D768[:3]
    probs = _make_group(M, shapes, gen)
    kinds, _ = _grouped(ops, M, probs, cus)
    assert kinds == [15]
    plain = [(q['dw'].m.clone(), q['db'].m.clone() if q['db'] is not None else None) for q in probs]
    prefill = []
    for q in probs:
        q['acc'] = 1
        pw = _rand(q['dw'].m.shape, torch.float32, 3.0, gen)
        q['dw'].m.copy_(pw)
        pb = None
        if q['db'] is not None:
            pb = _rand(q['db'].m.shape, torch.float32, 3.0, gen)
            q['db'].m.copy_(pb)
        prefill.append((pw, pb))
    kinds, _ = _grouped(ops, M, probs, cus)
    assert kinds == [15]
    for i, (q, (pw, pb), (w0, b0)) in enumerate(zip(probs, prefill, plain)):
        assert torch.equal(q['dw'].m, pw + w0), f'problem {i}: dW != prefill + the accumulate=0 result'
        assert q['dw'].untouched()
        if pb is not None:
            assert torch.equal(q['db'].m, pb + b0), f'problem {i}: db != prefill + the accumulate=0 result'


@gpu
@pytest.mark.parametrize('what', ['n_mod_256', 'm_below_64', 'thirteen_problems', 'grant_too_small'])
def test_grouped_refusals_leave_outputs_alone(ops, what):
    """A group the planner cannot take gets -1 from the workspace query and an error from the call; nothing is written."""
    L, lib = ops.L, ops.lib
    gen = torch.Generator(device='cuda').manual_seed(3)
    M, cus, shapes = 256, 0, [(256, 256, False, True)]
    if what == 'n_mod_256':
        shapes = [(256, 256, False, True), (264, 256, False, True)]
    elif what == 'm_below_64':
        M = 63
    elif what == 'thirteen_problems':
        shapes = [(256, 256, False, True)] * 13
    else:                      # 126 tiles on 8 CUs: 16 whole rounds, more than the 8 phases a plan may have
        shapes, cus = D768, 8
    probs = _make_group(M, shapes, gen)
    for q in probs:
        q['dw'].m.fill_(1.25)
        if q['db'] is not None:
            q['db'].m.fill_(-2.5)
    arr = _prob_array(L, probs)
    assert lib.egv_gemm_wgrad_grouped_workspace_bytes(M, len(probs), arr, cus) == -1
    ws = torch.empty(1 << 20, dtype=torch.uint8, device='cuda')
    kinds, rc = kinds_of(ops, lambda: lib.egv_gemm_wgrad_grouped(L.EGV_BF16, M, len(probs), arr, cus, ws.data_ptr(), 1 << 20, ops._st()))
    torch.cuda.synchronize()
    assert rc != 0 and kinds == []
    for q in probs:
        assert bool((q['dw'].m == 1.25).all()) and q['dw'].untouched()
        if q['db'] is not None:
            assert bool((q['db'].m == -2.5).all()) and q['db'].untouched()
