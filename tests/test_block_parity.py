"""Block-level parity of the two fused C-ABI calls nearly all of a step runs in -- egv_vblock_* (SpaceTimeBlock) and egv_tlayer_*
(RobertaLayer), csrc/egv_block.cpp -- against oracle/ref_model.py's own block (video_block, text_layer, and for the CLS-only head
form a restatement of video_transformer.py:217-219, :120 from its pieces) run in fp64 on the CPU with autograd, in the forms
bench.py and training run: the fp32 residual streams of the bf16 mode (EGV_VIDEO_RES32, EGV_TEXT_RES32), the LayerNorm fold between
two blocks, the head form of the last block, the text layer with train-mode dropout, and the ViT-L / RoBERTa-large width.

Weights are make_state_dict's, under the reference names, ordered as FrozenInTime._block_params orders them; inputs and upstream
gradients are random.  The output and EVERY gradient tensor are compared one by one (dx, dy / d_enc, each weight, bias, LayerNorm
term and gate; not the key biases, whose true gradient is exactly zero), and the CLS rows of the video output and of dx on their own
as well: they are the only rows the losses read, and a slip confined to them is invisible in the whole-tensor norm.

Bounds (relative L2 against the fp64 oracle on the same dtype-rounded inputs):
  fp32  5e-5 forward, 2e-4 gradients.
  bf16  the project's yardstick: the same oracle block run the way the reference's trainer runs it -- CUDA
        autocast, trainer_egoclip.py:143: Linear / matmul operands in bf16 and their results rounded to bf16; LayerNorm, softmax and
        the residual sums in fp32 (_Mixed below) -- against its own fp32 values.  Each tensor: error <= 1.5 x max(that tensor's
        yardstick error, the yardstick error of the whole gradient); tensors under 4096 elements (biases, LayerNorm terms) get 2^-9
        on top.
        The activations and the gradients of the block inputs (out, dx, dy / dhid / d_enc, qkv_s and their CLS rows) must also be free
        of a systematic gain: g = <kernel, oracle> / <oracle, oracle> within max(1.5 x the yardstick's |g - 1|, 2^-9) of 1.  Rounding
        noise hardly moves g (it is nearly orthogonal to the values), a scale slip moves it by its full size: a 2^-7 slip on the
        CLS rows of dx hides inside their bf16 noise (the yardstick's own relative error there is 1.2-2e-2) but not here.  Measured
        on the MI355X: |g - 1| <= 8.7e-4, at most 0.44 of its bound (dx[CLS] of the LayerNorm-fold chain).
The gates alpha_i2t / alpha_t2i are compared in absolute terms: their gradient is ONE sum over all rows, sum(dA * c) (c the gated
branch, dA the gradient of the sum it is added to), that cancels down to a small fraction of its terms, so its error is taken
relative to the size of those terms, ||dA * c||_2 (fp64 oracle), not to the sum itself (whose relative error is a single draw of the
rounding noise: measured that way, the kernel's came out at up to 2.5 x the yardstick's draw on the MI355X, in both directions).
torch.autocast('cpu') cannot serve as the yardstick: it returns softmax and layer_norm in bf16 for bf16 inputs, where CUDA autocast
keeps them in fp32.
"""

import pytest
import torch
import torch.nn.functional as F
from torch.overrides import TorchFunctionMode

import helpers  # noqa: F401  (caps the CPU oracle's threads)
from egovlpv2_amd.config import PathConfig
from egovlpv2_amd.synthetic import make_state_dict
from oracle import ref_model as O

bf16 = torch.bfloat16
F32_MIN = torch.finfo(torch.float32).min
FP32_FWD, FP32_BWD = 5e-5, 2e-4
SMALL = 4096                     # tensors below this many elements get the 2^-9 floor in bf16
FLOOR = 2.0 ** -9
GAIN_FLOOR = 2.0 ** -9           # systematic gain error below half a bf16 ulp is not flagged

# B, frames, img, patch (-> N space tokens per frame), width, heads, text tokens
GEOMS = {
    'small': dict(B=2, Fr=4, img=112, patch=16, dim=768, heads=12, L=16),       # N = 49, S = 197
    'ragged': dict(B=3, Fr=3, img=144, patch=16, dim=768, heads=12, L=45),      # N = 81, S = 244; B*S, N, L not multiples of 64
    'base': dict(B=1, Fr=16, img=224, patch=16, dim=768, heads=12, L=32),       # N = 196, S = 3137: the training step's block
    'vitl': dict(B=1, Fr=16, img=224, patch=14, dim=1024, heads=16, L=40),      # ViT-L/14, RoBERTa-large width: N = 256, MLP 4096
}


def _setup(geom, wseed=0):
    g = GEOMS[geom]
    pc = PathConfig(depth=2, n_fuse=1, img=g['img'], patch=g['patch'], frames=g['Fr'], dim=g['dim'], heads=g['heads'],
                    vocab=16, proj_dim=16)
    return g, pc, O.make_cfg(**pc.as_dict()), make_state_dict(pc, wseed)


# ---- parameter order of the block entry points (model.FrozenInTime._block_params, hipops.VideoBlockFn / TextLayerFn) ----------------
def video_names(i, fused):
    pfx = f'video_model.blocks.{i}'
    names = [f'{pfx}.{m}.{t}' for m in ('timeattn.qkv', 'timeattn.proj', 'attn.qkv', 'attn.proj', 'mlp.fc1', 'mlp.fc2')
             for t in ('weight', 'bias')]
    names += [f'{pfx}.{m}.{t}' for m in ('norm3', 'norm1', 'norm2') for t in ('weight', 'bias')]
    if fused:
        a = pfx + '.attn'
        names += [f'{a}.{m}.{t}' for m in ('qkv_text_i2t', 'qkv_i2t', 'proj_i2t') for t in ('weight', 'bias')]
        names += [a + '.norm_i2t_i.weight', a + '.norm_i2t_i.bias', a + '.alpha_i2t']
    return names


def head_names(i):
    """VideoHeadFn: [W, b] of timeattn.qkv, timeattn.proj, attn.qkv, then norm3, norm1 (model._video_tail_head)"""
    v = video_names(i, False)
    return v[0:6] + v[12:16]


def text_names(i, fused):
    pfx = f'text_model.encoder.layer.{i}'
    names = [f'{pfx}.{m}.{t}' for m in ('attention.self.query', 'attention.self.key', 'attention.self.value',
                                       'attention.output.dense', 'intermediate.dense', 'output.dense') for t in ('weight', 'bias')]
    names += [f'{pfx}.{m}.{t}' for m in ('attention.output.LayerNorm', 'output.LayerNorm') for t in ('weight', 'bias')]
    if fused:
        ca = pfx + '.crossattention_t2i'
        names += [f'{ca}.{m}.{t}' for m in ('self.query', 'self.key', 'self.value', 'output.dense') for t in ('weight', 'bias')]
        names += [pfx + '.alpha_t2i']
    return names


# ---- the oracle in the precision policy of CUDA autocast ---------------------------------------------------------------------------
class _Mixed(TorchFunctionMode):
    """Runs oracle/ref_model.py's plain functional torch under a precision policy and with dropout masks.

    mixed=True: what CUDA autocast does to the ops the blocks use -- F.linear and matmul on bf16 operands with a bf16 result (CPU bf16
    GEMMs accumulate in fp32, as the GPU's do; their backward runs in bf16 too), softmax and layer_norm in fp32 with an fp32 result;
    everything else in the dtype torch's promotion gives it, so a residual sum with an fp32 operand is fp32.
    drop_lin: {id(weight): multiplier} -- hidden-state dropout on that Linear's output (RobertaSelfOutput / RobertaOutput: dense ->
    dropout, roberta.py:342, :422); drop_attn: multipliers of the softmax results in call order (roberta.py:313).
    capture: {id(weight): key} -- keep that Linear's output (after dropout) and its gradient in `captured[key]`."""

    def __init__(self, mixed=False, drop_lin=None, drop_attn=(), capture=None):
        super().__init__()
        self.mixed, self.drop_lin, self.drop_attn = mixed, drop_lin or {}, list(drop_attn)
        self.capture, self.captured = capture or {}, {}

    def __torch_function__(self, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        if func is F.linear:
            x, w = args[0], args[1]
            b = args[2] if len(args) > 2 else kwargs.get('bias')
            if self.mixed:
                out = F.linear(x.to(bf16), w.to(bf16), None if b is None else b.to(bf16))
            else:
                out = F.linear(x, w, b)
            m = self.drop_lin.get(id(w))
            out = out if m is None else out * m.to(out.dtype)
            if id(w) in self.capture:
                out.retain_grad()
                self.captured[self.capture[id(w)]] = out
            return out
        if func in (torch.matmul, torch.Tensor.matmul, torch.Tensor.__matmul__) and self.mixed:
            return torch.matmul(args[0].to(bf16), args[1].to(bf16))
        if func in (torch.softmax, torch.Tensor.softmax, F.softmax):
            x, dim = args[0], (args[1] if len(args) > 1 else kwargs['dim'])
            out = torch.softmax(x.float() if self.mixed else x, dim)
            if self.drop_attn:
                out = out * self.drop_attn.pop(0).to(out.dtype)
            return out
        if func is F.layer_norm and self.mixed:
            args = [a.float() if torch.is_tensor(a) else a for a in args]
            return F.layer_norm(*args, **kwargs)
        return func(*args, **kwargs)


def _leaves(ts, dtype):
    return [t.detach().to(dtype).clone().requires_grad_(True) for t in ts]


# gate -> the Linear whose output it scales (video_transformer.py:185, roberta.py:486)
GATES = {'.attn.alpha_i2t': '.attn.proj_i2t.weight', '.alpha_t2i': '.crossattention_t2i.output.dense.weight'}


def _oracle(fn, names, P, inputs, douts, dtype, mixed=False, drop=None):
    """run fn(sd, *inputs) -> outputs on CPU leaves of `dtype` built from the block's parameter list P (entry-point order, mapped back
    to the reference names) and inputs; backward with douts.  Returns (outputs, input grads, parameter grads in P's order,
    {gate name: ||dA * c||_2, the size of the terms of its gradient})."""
    Pl = _leaves(P, dtype)
    sd = dict(zip(names, Pl))
    xs = [None if t is None else t.detach().to(dtype).clone().requires_grad_(t.is_floating_point()) for t in inputs]
    drop_lin, drop_attn = {}, ()
    if drop is not None:
        drop_lin = {id(sd[n]): m for n, m in drop[0].items()}
        drop_attn = drop[1]
    gates = {n: n[:-len(k)] + v for n in names for k, v in GATES.items() if n.endswith(k)}
    mode = _Mixed(mixed, drop_lin, drop_attn, capture={id(sd[w]): n for n, w in gates.items()})
    with mode:
        outs = fn(sd, *xs)
    outs = outs if isinstance(outs, tuple) else (outs,)
    torch.autograd.backward([o for o in outs], [d.to(o.dtype) for o, d in zip(outs, douts)])
    scale = {}
    for n, c in mode.captured.items():        # c's gradient is alpha * dA
        scale[n] = ((c.grad.double() * c.detach().double()).norm() / sd[n].detach().double().abs()).item()
    return ([o.detach() for o in outs], [None if (x is None or not x.requires_grad) else x.grad for x in xs],
            [p.grad if p.grad is not None else torch.zeros_like(p) for p in Pl], scale)


# ---- comparison -----------------------------------------------------------------------------------------------------------------------
def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _err(k, r, scale):
    if scale is None:
        return _rel(k, r)
    return (k.detach().double().cpu() - r.detach().double().cpu()).norm().item() / scale


def _gain(k, r):
    k, r = k.detach().double().cpu().reshape(-1), r.detach().double().cpu().reshape(-1)
    return (k @ r / (r @ r).clamp_min(1e-300)).item()


def _compare(label, items, precision):
    """items: (name, kernel, fp64 oracle, mixed-precision oracle or None, is_gradient, absolute scale or None).  fp32: fixed
    bounds; bf16: the yardstick.  Returns the worst kernel / yardstick ratio (bf16) or the worst error (fp32) and prints it."""
    bad, worst = [], (0.0, '')
    items = [it if len(it) == 6 else it + (None,) for it in items]
    if precision == 'fp32':
        for name, k, r, _, grad, sc in items:
            e, lim = _err(k, r, sc), (FP32_BWD if grad else FP32_FWD)
            worst = max(worst, (e, name))
            if not e <= lim:
                bad.append(f'{name}: {e:.3e} > {lim:.1e}')
    else:
        g64 = torch.cat([r.detach().double().cpu().reshape(-1) for _, _, r, _, grad, _ in items if grad])
        gac = torch.cat([a.detach().double().cpu().reshape(-1) for _, _, _, a, grad, _ in items if grad])
        e_all = ((gac - g64).norm() / g64.norm()).item()
        for name, k, r, a, grad, sc in items:
            e, ey = _err(k, r, sc), _err(a, r, sc)
            base = max(ey, e_all)
            lim = 1.5 * base + (FLOOR if (r.numel() < SMALL and sc is None) else 0.0)
            worst = max(worst, (e / base, name))
            if not e <= lim:
                bad.append(f'{name}: {e:.3e} > {lim:.3e} (yardstick {ey:.3e}, whole gradient {e_all:.3e})')
            if not name.startswith('d ') and sc is None:          # activations and input gradients: no systematic gain
                gk, gy = _gain(k, r), _gain(a, r)
                if not abs(gk - 1) <= max(1.5 * abs(gy - 1), GAIN_FLOOR):
                    bad.append(f'{name}: gain {gk:.6f} (yardstick {gy:.6f})')
    print(f'\n[block parity] {label}: worst {"error" if precision == "fp32" else "kernel/yardstick"} {worst[0]:.3g} ({worst[1]})')
    assert not bad, f'{label}:\n  ' + '\n  '.join(bad)
    return worst[0]


def _items(pfx, names, kg, g64, gac, scale):
    out = []
    for n, k, r, a in zip(names, kg, g64, gac if gac is not None else [None] * len(names)):
        if n.endswith('.key.bias'):
            continue
        out.append((pfx + n, k, r, a, True, scale.get(n)))
    return out


def _text_mask(B, L):
    """additive (B, L) key mask: sample 0 has a padded tail, sample 1 (if any) a single valid token"""
    m = torch.ones(B, L)
    m[0, L - L // 3:] = 0
    if B > 1:
        m[1, 1:] = 0
    return ((1 - m) * F32_MIN).contiguous()


def _rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


@pytest.fixture(scope='module')
def ops():
    from egovlpv2_amd import hipops
    return hipops


# ---- video block ----------------------------------------------------------------------------------------------------------------------
def _video_ref(i, cfg, B, S, fused):
    def fn(sd, x, y=None, m=None):
        D = x.shape[-1]
        out = O.video_block(x.view(B, S, D), i, sd, cfg, y=None if y is None else y.view(B, -1, D), y_mask_add=m)
        return out.reshape(B * S, D)
    return fn


# (form, fused, geometry): every form meets every geometry, each form both unfused and fused
VIDEO_CASES = [('fp32', False, 'small'), ('fp32', True, 'ragged'), ('fp32', False, 'base'), ('fp32', True, 'vitl'),
               ('bf16', True, 'small'), ('bf16', False, 'ragged'), ('bf16', True, 'base'), ('bf16', False, 'vitl'),
               ('res32', False, 'small'), ('res32', True, 'small'), ('res32', True, 'ragged'), ('res32', True, 'base'),
               ('res32', False, 'base'), ('res32', False, 'vitl')]


@pytest.mark.gpu
@pytest.mark.parametrize('form,fused,geom', VIDEO_CASES)
def test_video_block_vs_fp64_oracle(ops, form, fused, geom, monkeypatch):
    """ops.video_block forward + backward in fp32, bf16 with the bf16 residual stream (EGV_VIDEO_RES32=0) and bf16 with the fp32
    stream (the bf16 default: stream32 output and dx), unfused and fused with a padded text mask.
    Measured on the MI355X, worst tensor of each case: fp32 <= 5.7e-6 (ViT-L timeattn.qkv weight gradient); kernel / yardstick
    0.93 - 1.42 with EGV_VIDEO_RES32=0 (1.42: alpha_i2t in absolute terms at the full base shape; every other tensor <= 0.99), 0.87 -
    1.02 with the fp32 stream (1.02: alpha_i2t, ragged; dx[CLS] 0.87 - 0.89)."""
    g, pc, cfg, sd = _setup(geom)
    B, L, D = g['B'], g['L'], g['dim']
    S, H, Hd, eps = cfg.seq, cfg.heads, D * cfg.mlp_ratio, cfg.eps_video
    i = 1 if fused else 0
    names = video_names(i, fused)
    P = [sd[n] for n in names]
    monkeypatch.setenv('EGV_VIDEO_RES32', '0' if form == 'bf16' else '1')
    dt = torch.float32 if form == 'fp32' else bf16
    x32 = _rnd((B * S, D), 11)
    x_in = x32 if form in ('fp32', 'res32') else x32.to(bf16).float()          # what the block reads as its input
    y = _rnd((B * L, D), 12).to(dt) if fused else None
    mask = _text_mask(B, L) if fused else None
    dout = _rnd((B * S, D), 13).to(dt)

    ops.begin_step()
    Pk = [p.cuda().requires_grad_(True) for p in P]
    x = x32.to(dt).cuda().requires_grad_(True)
    if form == 'res32':
        x._res32 = x32.cuda()
    yk = y.cuda().requires_grad_(True) if fused else None
    out = ops.video_block(x, Pk, B, cfg.frames, cfg.n_patches, H, Hd, eps, y=yk, y_mask=mask.cuda() if fused else None, L=L if fused else 0)
    o = ops.stream32(out) if form == 'res32' else out
    assert (o is not None) and o.dtype == (torch.float32 if form != 'bf16' else bf16)
    if form == 'res32':
        assert torch.equal(out, o.to(bf16))
    out.backward(dout.cuda())
    torch.cuda.synchronize()

    fn = _video_ref(i, cfg, B, S, fused)
    inputs = [x_in, y, mask] if fused else [x_in]
    (o64,), gi64, gp64, sc64 = _oracle(fn, names, P, inputs, [dout], torch.float64)
    oac = giac = gpac = None
    if form != 'fp32':
        (oac,), giac, gpac, _ = _oracle(fn, names, P, inputs, [dout], torch.float32, mixed=True)
    cls = lambda t: None if t is None else t.reshape(B, S, D)[:, 0]          # noqa: E731
    items = [('out', o, o64, oac, False), ('out[CLS]', cls(o), cls(o64), cls(oac), False),
             ('dx', x.grad, gi64[0], None if giac is None else giac[0], True),
             ('dx[CLS]', cls(x.grad), cls(gi64[0]), cls(None if giac is None else giac[0]), True)]
    if fused:
        items.append(('dy', yk.grad, gi64[1], None if giac is None else giac[1], True))
    items += _items('d ', names, [p.grad for p in Pk], gp64, gpac, sc64)
    _compare(f'video {form} {"fused" if fused else "unfused"} {geom}', items, 'fp32' if form == 'fp32' else 'bf16')


@pytest.mark.gpu
@pytest.mark.parametrize('geom', ['small', 'ragged'])
def test_video_layernorm_fold_chain_vs_fp64_oracle(ops, geom):
    """Two consecutive fp32-stream blocks (EGV_VIDEO_RES32, the bf16 default): the first is called with next_ln and writes the second
    block's norm3 in its output pass (EGV_LN_FOLD, BLOCK_H3_READY); the second is fused.  Both blocks' gradients, dx, dy and the
    output against the fp64 two-block chain.  Measured on the MI355X: kernel / yardstick <= 0.93 (norm3 / norm1 weight gradients)."""
    g, pc, cfg, sd = _setup(geom)
    B, L, D = g['B'], g['L'], g['dim']
    S, H, Hd, eps = cfg.seq, cfg.heads, D * cfg.mlp_ratio, cfg.eps_video
    n0, n1 = video_names(0, False), video_names(1, True)
    P0, P1 = [sd[n] for n in n0], [sd[n] for n in n1]
    x32 = _rnd((B * S, D), 21)
    y = _rnd((B * L, D), 22).to(bf16)
    mask = _text_mask(B, L)
    dout = _rnd((B * S, D), 23).to(bf16)

    ops.begin_step()
    K0, K1 = [p.cuda().requires_grad_(True) for p in P0], [p.cuda().requires_grad_(True) for p in P1]
    x = x32.to(bf16).cuda().requires_grad_(True)
    x._res32 = x32.cuda()
    yk = y.cuda().requires_grad_(True)
    mid = ops.video_block(x, K0, B, cfg.frames, cfg.n_patches, H, Hd, eps, next_ln=(K1[12], K1[13], L, False))
    assert '_pre_save' in mid.__dict__, 'the first block did not fold the next LayerNorm'
    out = ops.video_block(mid, K1, B, cfg.frames, cfg.n_patches, H, Hd, eps, y=yk, y_mask=mask.cuda(), L=L)
    assert '_pre_save' not in mid.__dict__, 'the second block did not take the folded LayerNorm'
    o = ops.stream32(out)
    out.backward(dout.cuda())
    torch.cuda.synchronize()

    f0, f1 = _video_ref(0, cfg, B, S, False), _video_ref(1, cfg, B, S, True)

    def chain(sd_, x_, y_, m_):
        return f1(sd_, f0(sd_, x_), y_, m_)
    names, P = n0 + n1, P0 + P1
    (o64,), gi64, gp64, sc64 = _oracle(chain, names, P, [x32, y, mask], [dout], torch.float64)
    (oac,), giac, gpac, _ = _oracle(chain, names, P, [x32, y, mask], [dout], torch.float32, mixed=True)
    cls = lambda t: t.reshape(B, S, D)[:, 0]                                 # noqa: E731
    items = [('out', o, o64, oac, False), ('out[CLS]', cls(o), cls(o64), cls(oac), False),
             ('dx', x.grad, gi64[0], giac[0], True), ('dx[CLS]', cls(x.grad), cls(gi64[0]), cls(giac[0]), True),
             ('dy', yk.grad, gi64[1], giac[1], True)]
    items += _items('d ', names, [p.grad for p in K0 + K1], gp64, gpac, sc64)
    _compare(f'video LayerNorm-fold chain {geom}', items, 'bf16')


@pytest.mark.gpu
@pytest.mark.parametrize('geom', ['small', 'ragged', 'base', 'vitl'])
def test_video_block_head_vs_fp64_oracle(ops, geom):
    """ops.video_block_head, the all-rows part of the CLS-only last block (EGV_BLOCK_HEAD): qkv_s over all rows, the fp32 CLS rows of
    the input, and the gradients of its 10 parameters and of x, against the fp64 restatement of video_transformer.py:217-219, :120
    (norm3, time attention + projection + residual, norm1, attn.qkv) and the space residual's CLS rows (:222).
    Measured on the MI355X: kernel / yardstick 0.94 - 1.04 (dx[CLS])."""
    g, pc, cfg, sd = _setup(geom)
    B, D = g['B'], g['dim']
    S, H, Hd, eps = cfg.seq, cfg.heads, D * cfg.mlp_ratio, cfg.eps_video
    names = head_names(0)
    P = [sd[n] for n in names]
    x32 = _rnd((B * S, D), 31)
    dq = _rnd((B * S, 3 * D), 32).to(bf16)
    dxc = _rnd((B, D), 33)

    ops.begin_step()
    Pk = [p.cuda().requires_grad_(True) for p in P]
    x = x32.to(bf16).cuda().requires_grad_(True)
    x._res32 = x32.cuda()
    qkv, xc = ops.video_block_head(x, Pk, B, cfg.frames, cfg.n_patches, H, Hd, eps)
    assert qkv.shape == (B * S, 3 * D) and qkv.dtype == bf16 and xc.shape == (B, D) and xc.dtype == torch.float32
    torch.autograd.backward([qkv, xc], [dq.cuda(), dxc.cuda()])
    torch.cuda.synchronize()

    def head(sd_, x_):
        p = 'video_model.blocks.0'
        xb = x_.view(B, S, D)
        t = O.divided_attention(O._ln(xb, sd_, p + '.norm3', eps), sd_, p + '.timeattn', cfg, 'time')
        q = O._lin(O._ln(xb + t, sd_, p + '.norm1', eps), sd_, p + '.attn.qkv')
        return q.reshape(B * S, 3 * D), xb[:, 0]
    (q64, xc64), gi64, gp64, sc64 = _oracle(head, names, P, [x32], [dq, dxc], torch.float64)
    (qac, xcac), giac, gpac, _ = _oracle(head, names, P, [x32], [dq, dxc], torch.float32, mixed=True)
    cls = lambda t: t.reshape(B, S, -1)[:, 0]                                # noqa: E731
    items = [('qkv_s', qkv, q64, qac, False), ('qkv_s[CLS]', cls(qkv), cls(q64), cls(qac), False), ('x[CLS] fp32', xc, xc64, xcac, False),
             ('dx', x.grad, gi64[0], giac[0], True), ('dx[CLS]', cls(x.grad), cls(gi64[0]), cls(giac[0]), True)]
    items += _items('d ', names, [p.grad for p in Pk], gp64, gpac, sc64)
    _compare(f'video head form {geom}', items, 'bf16')


# ---- text layer -----------------------------------------------------------------------------------------------------------------------
def _text_ref(i, cfg, B, L, S):
    def fn(sd, hid, m, enc=None):
        D = hid.shape[-1]
        out = O.text_layer(hid.view(B, L, D), m.view(B, 1, 1, L), i, sd, cfg, enc=None if enc is None else enc.view(B, S, D))
        return out.reshape(B * L, D)
    return fn


TEXT_CASES = [(form, fused, geom) for geom in GEOMS for form in ('fp32', 'bf16', 'res32') for fused in (False, True)]
SEEDS = (0x1234567, 0x2468ACE, 0x369CF12, 0x48D159E, 0x5A1B2C3)


def _hidden_keep(ops, which, n, p, seed):
    """the multiplier (0 or 1/(1-p)) of one hidden-state dropout site, from the entry point the text layer itself calls there:
    egv_dropout_add_mixed (bf16 -> fp32 stream) or egv_dropout_add (bf16) -- over n ones, no residuals"""
    import ctypes as C
    from egovlpv2_amd import _lib as L_
    ones = torch.ones(n, dtype=bf16, device='cuda')
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if which == 'mixed':
        y = torch.empty(n, dtype=torch.float32, device='cuda')
        rc = L_.lib.egv_dropout_add_mixed(L_.EGV_BF16, C.c_void_p(ones.data_ptr()), None, None, L_.EGV_F32, C.c_void_p(y.data_ptr()),
                                          n, p, seed, st)
    else:
        y = torch.empty(n, dtype=bf16, device='cuda')
        rc = L_.lib.egv_dropout_add(L_.EGV_BF16, C.c_void_p(ones.data_ptr()), None, None, C.c_void_p(y.data_ptr()), n, p, seed, st)
    assert rc == 0, L_.lib.egv_last_error()
    torch.cuda.synchronize()
    return y.double().cpu()


def _keep_mult(M, p):
    inv = 1.0 / (1.0 - p)
    on = (M - inv).abs() < 0.02 * inv
    assert bool((on | (M.abs() < 1e-6)).all()), 'multiplier is 0 or 1/(1-p)'
    assert abs(on.double().mean().item() - (1 - p)) < 0.02, on.double().mean().item()
    return on.double() * inv


def _dropout_masks(ops, B, L, S, H, D, p, seeds, fused):
    """the masks of the text layer's sites (seeds: 0 self-attention probabilities, 1 attention.output.dense, 2 cross-attention
    probabilities, 3 crossattention_t2i.output.dense, 4 output.dense; model._text_layer draws them in that order) -- hidden sites
    through the mask entry point the res32 layer calls (csrc/egv_block.cpp egv_tlayer_fwd), probability sites through the attention
    kernel itself at the layer's (B, H, nq, nk)"""
    from test_hip_ops import _attn_keep_mult
    n = B * L * D
    hid = {1: _hidden_keep(ops, 'plain' if fused else 'mixed', n, p, seeds[1]), 4: _hidden_keep(ops, 'mixed', n, p, seeds[4])}
    att = {0: _attn_keep_mult(ops, bf16, B, H, L, L, p, seeds[0])}
    if fused:
        hid[3] = _hidden_keep(ops, 'mixed', n, p, seeds[3])
        att[2] = _attn_keep_mult(ops, bf16, B, H, L, S, p, seeds[2])
    hid = {k: _keep_mult(v, p).view(B * L, D) for k, v in hid.items()}
    att = {k: _keep_mult(v, p) for k, v in att.items()}
    sites = list(hid.values()) + [a.reshape(-1) for a in att.values()]
    assert len(sites) == (5 if fused else 3)
    for a in range(len(sites)):
        for b in range(a + 1, len(sites)):
            k = min(sites[a].numel(), sites[b].numel())
            assert not torch.equal(sites[a].reshape(-1)[:k], sites[b].reshape(-1)[:k]), 'two dropout sites share a mask'
    return hid, att


def _text_case(ops, form, fused, geom, drop_p=0.0):
    g, pc, cfg, sd = _setup(geom)
    B, L, D = g['B'], g['L'], g['dim']
    S, H, Hd, eps = cfg.seq, cfg.heads, D * cfg.mlp_ratio, cfg.eps_text
    i = 1 if fused else 0
    names = text_names(i, fused)
    P = [sd[n] for n in names]
    dt = bf16 if form == 'bf16' else torch.float32                      # res32: hid / out are the fp32 stream
    res32 = form == 'res32'
    h32 = _rnd((B * L, D), 41)
    h_in = h32.to(dt).float()
    enc = _rnd((B * S, D), 42).to(torch.float32 if form == 'fp32' else bf16) if fused else None
    mask = _text_mask(B, L)
    dout = _rnd((B * L, D), 43).to(dt)
    seeds = tuple(SEEDS) + (0,) if drop_p > 0 else (0,) * 6

    ops.begin_step()
    Pk = [p.cuda().requires_grad_(True) for p in P]
    hid = h32.to(dt).cuda().requires_grad_(True)
    ek = enc.cuda().requires_grad_(True) if fused else None
    out = ops.text_layer(hid, mask.cuda(), Pk, B, L, H, Hd, eps, enc=ek, S=S if fused else 0, drop_p=drop_p, seeds=seeds, res32=res32)
    assert out.dtype == dt
    out.backward(dout.cuda())
    torch.cuda.synchronize()

    drop = None
    if drop_p > 0:
        hid_m, att_m = _dropout_masks(ops, B, L, S, H, D, drop_p, seeds, fused)
        pfx = f'text_model.encoder.layer.{i}'
        lin = {pfx + '.attention.output.dense.weight': hid_m[1], pfx + '.output.dense.weight': hid_m[4]}
        if fused:
            lin[pfx + '.crossattention_t2i.output.dense.weight'] = hid_m[3]
        drop = (lin, [att_m[0]] + ([att_m[2]] if fused else []))

    def dr(dtype):
        if drop is None:
            return None
        return ({k: v.view(B, L, D).to(dtype) for k, v in drop[0].items()}, [a.to(dtype) for a in drop[1]])
    fn = _text_ref(i, cfg, B, L, S)
    inputs = [h_in, mask] + ([enc] if fused else [])
    (o64,), gi64, gp64, sc64 = _oracle(fn, names, P, inputs, [dout], torch.float64, drop=dr(torch.float64))
    oac = giac = gpac = None
    if form != 'fp32':
        (oac,), giac, gpac, _ = _oracle(fn, names, P, inputs, [dout], torch.float32, mixed=True, drop=dr(torch.float32))
    items = [('out', out, o64, oac, False), ('dhid', hid.grad, gi64[0], None if giac is None else giac[0], True)]
    if fused:
        items.append(('denc', ek.grad, gi64[2], None if giac is None else giac[2], True))
    items += _items('d ', names, [p.grad for p in Pk], gp64, gpac, sc64)
    return _compare(f'text {form} {"fused" if fused else "unfused"} {geom}{" dropout %.2g" % drop_p if drop_p else ""}', items,
                    'fp32' if form == 'fp32' else 'bf16')


@pytest.mark.gpu
@pytest.mark.parametrize('form,fused,geom', TEXT_CASES)
def test_text_layer_vs_fp64_oracle(ops, form, fused, geom):
    """ops.text_layer forward + backward in fp32, bf16 and bf16 with the fp32 residual stream (res32: EGV_TEXT_RES32, the bf16
    default; egv_layernorm_fwd_res32 / _bwd_res32 and the mixed-type residual sums), unfused and fused over S = 197 ... 4097 video
    tokens, with a padded tail and a single-token caption in the key mask.  Measured on the MI355X, worst tensor of each case:
    fp32 <= 2.0e-6; kernel / yardstick 0.88 - 1.13 in bf16 (1.13: alpha_t2i in absolute terms, ragged; d_enc 1.02), 0.88 - 0.95
    with res32."""
    _text_case(ops, form, fused, geom)


@pytest.mark.gpu
@pytest.mark.parametrize('fused,geom', [(False, 'small'), (True, 'small'), (True, 'base')])
def test_text_layer_dropout_vs_fp64_oracle(ops, fused, geom):
    """What a training step runs: the res32 text layer with drop_p = 0.1 (bench.py --drop-rate; roberta-base's hidden and attention
    dropout).  The masks are recovered from the entry points the layer calls with its own seeds and element counts / (B, H, nq, nk) and
    applied in the oracle: keep rate within 0.02 of 0.9 at every site, no two sites (three unfused, five fused) with one mask.
    Measured on the MI355X: kernel / yardstick 0.88 - 0.91."""
    _text_case(ops, 'res32', fused, geom, drop_p=0.1)


# ---- CPU: the reference plumbing -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['video', 'video_fused', 'head', 'text', 'text_fused_dropout'])
def test_oracle_block_plumbing_fp32_vs_fp64(kind):
    """Without a GPU: the harness above (entry-point parameter order mapped back to the reference names, the views, the dropout
    masks of _Mixed, the head restatement) run in fp32 against itself in fp64 -- every output and gradient within 1e-5 -- and the
    mixed-precision yardstick runs and lands at bf16-sized errors, neither 0 nor O(1)."""
    g, pc, cfg, sd = _setup('small')
    B, L, D = g['B'], g['L'], g['dim']
    S = cfg.seq
    mask = _text_mask(B, L)
    if kind.startswith('video') or kind == 'head':
        fused = kind == 'video_fused'
        names = head_names(0) if kind == 'head' else video_names(1 if fused else 0, fused)
        if kind == 'head':
            def fn(sd_, x_):
                p = 'video_model.blocks.0'
                xb = x_.view(B, S, D)
                t = O.divided_attention(O._ln(xb, sd_, p + '.norm3', 1e-5), sd_, p + '.timeattn', cfg, 'time')
                return O._lin(O._ln(xb + t, sd_, p + '.norm1', 1e-5), sd_, p + '.attn.qkv').reshape(B * S, 3 * D)
            douts = [_rnd((B * S, 3 * D), 3)]
        else:
            fn = _video_ref(1 if fused else 0, cfg, B, S, fused)
            douts = [_rnd((B * S, D), 3)]
        inputs = [_rnd((B * S, D), 1)] + ([_rnd((B * L, D), 2), mask] if fused else [])
        drop = None
    else:
        fused = kind == 'text_fused_dropout'
        names = text_names(1 if fused else 0, fused)
        fn = _text_ref(1 if fused else 0, cfg, B, L, S)
        inputs = [_rnd((B * L, D), 1), mask] + ([_rnd((B * S, D), 2)] if fused else [])
        douts = [_rnd((B * L, D), 3)]
        drop = None
        if fused:
            gen = torch.Generator().manual_seed(5)
            km = lambda *s: (torch.rand(*s, generator=gen) >= 0.1).double() / 0.9          # noqa: E731
            pfx = 'text_model.encoder.layer.1'
            drop = ({pfx + n: km(B, L, D) for n in ('.attention.output.dense.weight', '.output.dense.weight',
                                                    '.crossattention_t2i.output.dense.weight')},
                    [km(B, cfg.heads, L, L), km(B, cfg.heads, L, S)])
    P = [sd[n] for n in names]
    cast = lambda d, t: None if d is None else ({k: v.to(t) for k, v in d[0].items()}, [a.to(t) for a in d[1]])   # noqa: E731
    o64, gi64, gp64, sc64 = _oracle(fn, names, P, inputs, douts, torch.float64, drop=cast(drop, torch.float64))
    o32, gi32, gp32, _ = _oracle(fn, names, P, inputs, douts, torch.float32, drop=cast(drop, torch.float32))
    oac, _, gpac, _ = _oracle(fn, names, P, inputs, douts, torch.float32, mixed=True, drop=cast(drop, torch.float32))
    assert ('alpha' in ' '.join(names)) == bool(sc64) and all(v > 0 for v in sc64.values())
    pairs = list(zip(o32, o64)) + [(a, b) for a, b in zip(gi32, gi64) if b is not None]
    pairs += [(a, b) for n, a, b in zip(names, gp32, gp64) if not n.endswith('.key.bias')]
    for a, b in pairs:
        assert _rel(a, b) < 1e-5, (kind, _rel(a, b))
    e = _rel(oac[0], o64[0])
    assert 1e-4 < e < 3e-2, e
    eg = max(_rel(a, b) for n, a, b in zip(names, gpac, gp64) if not n.endswith('.key.bias'))
    assert 1e-4 < eg < 0.2, eg
    if drop is not None:                        # the masks reach the oracle: without them the result moves far
        o_nd, _, _, _ = _oracle(fn, names, P, inputs, douts, torch.float64)
        assert _rel(o_nd[0], o64[0]) > 1e-2
