"""Stochastic depth (drop_path_rate) of the fine-tune variant's video blocks -- reference model_epic_charades.py:83 ->
SpaceTimeTransformer (video_transformer.py:297: rates linspace(0, drop_path_rate, depth)) -> SpaceTimeBlock (:206, :222, :226: timm
DropPath on the space branch and on the MLP branch, per sample; the time branch is never scaled).

The reference for the GPU tests is the pinned oracle's own pieces (O._ln, O.divided_attention, O._lin, O._gelu) composed into the
drop-path block, with the multipliers applied exactly where :222 / :226 apply them; block-level comparisons reuse the harness and the
bounds of test_block_parity.py (fp32 5e-5 / 2e-4, bf16 1.5 x the autocast yardstick with its gain check), model-level ones the
tolerances of test_model_parity.py::test_dual_finetune_variant_vs_golden.
"""
import inspect
import math
import types

import pytest
import torch

import helpers  # noqa: F401  (caps the CPU oracle's threads)
import test_block_parity as T
from helpers import load_golden_dual, dual_batch
from oracle import ref_model as O

bf16 = torch.bfloat16
KEEP = 0.8                                    # multipliers of the block tests: 0 or 1 / KEEP (1.25: exact in bf16)
# B = 4 samples, one in each keep / drop combination of (space branch, MLP branch)
M_ATTN = torch.tensor([1 / KEEP, 0.0, 1 / KEEP, 0.0])
M_MLP = torch.tensor([1 / KEEP, 1 / KEEP, 0.0, 0.0])


def dp_video_block(x, i, sd, cfg, m_attn, m_mlp):
    """SpaceTimeBlock.forward (video_transformer.py:214-228) with DropPath: sr = x + m_attn[b] * space (:222, base x), out = sr +
    m_mlp[b] * mlp (:226); x is (B, S, D), m_* are (B,)"""
    p = f'video_model.blocks.{i}'
    eps = cfg.eps_video
    B = x.shape[0]
    t = O.divided_attention(O._ln(x, sd, p + '.norm3', eps), sd, p + '.timeattn', cfg, 'time')
    tr = x + t
    s = O.divided_attention(O._ln(tr, sd, p + '.norm1', eps), sd, p + '.attn', cfg, 'space')
    sr = x + m_attn.view(B, 1, 1).to(s.dtype) * s
    h = O._lin(O._gelu(O._lin(O._ln(sr, sd, p + '.norm2', eps), sd, p + '.mlp.fc1')), sd, p + '.mlp.fc2')
    return sr + m_mlp.view(B, 1, 1).to(h.dtype) * h


# ---- CPU: the reference plumbing and the missing feature ----------------------------------------------------------------------------
def test_composed_block_matches_oracle_and_drops_to_identity():
    g, pc, cfg, sd = T._setup('small')
    B, S, D = 2, cfg.seq, g['dim']
    x = T._rnd((B, S, D), 5)
    ones = torch.ones(B)
    with torch.no_grad():
        ref = O.video_block(x, 0, sd, cfg)
        assert torch.equal(dp_video_block(x, 0, sd, cfg, ones, ones), ref)
        z = torch.tensor([1.0, 0.0])
        out = dp_video_block(x, 0, sd, cfg, z, z)
    assert torch.equal(out[1], x[1])                    # both branches dropped: the input rows themselves
    assert torch.equal(out[0], ref[0])


def test_finetune_variant_accepts_drop_path_rate():
    from egovlpv2_amd.model.model_epic_charades import FrozenInTime
    from egovlpv2_amd.config import tiny_config
    import dataclasses
    cfg = dataclasses.replace(tiny_config(), proj_dim=256, proj_style='linear')
    m = FrozenInTime({'model': 'SpaceTimeTransformer', 'num_frames': cfg.frames, 'pretrained': True, 'drop_path_rate': 0.1},
                     {'model': 'roberta-base', 'pretrained': True, 'input': 'text'}, path_config=cfg, compute_dtype=torch.float32)
    ref = [r.item() for r in torch.linspace(0, 0.1, cfg.depth)]
    assert m._dp_rates == ref and m._dp_rates[0] == 0.0 and m.drop_path_rate == 0.1
    m0 = FrozenInTime({'model': 'SpaceTimeTransformer', 'num_frames': cfg.frames, 'pretrained': True, 'drop_path_rate': 0.0},
                      {'model': 'roberta-base', 'pretrained': True, 'input': 'text'}, path_config=cfg, compute_dtype=torch.float32)
    assert m0._dp_rates is None
    with pytest.raises(ValueError):
        FrozenInTime({'model': 'SpaceTimeTransformer', 'num_frames': cfg.frames, 'drop_path_rate': 1.0},
                     {'model': 'roberta-base', 'input': 'text'}, path_config=cfg, compute_dtype=torch.float32)


def test_video_block_and_abi_carry_the_multipliers():
    from egovlpv2_amd import hipops as ops
    from egovlpv2_amd import _lib as L
    assert 'dp_scale' in inspect.signature(ops.video_block).parameters
    assert callable(ops.drop_path_scales)
    assert L.VBlockDesc._fields_[-1][0] == 'dp_scale'
    assert L.lib.egv_abi_version() == 7


# ---- GPU: block level -----------------------------------------------------------------------------------------------------------------
def _run_block(ops, P, x32, form, B, cfg, dout, dp):
    g_dt = torch.float32 if form == 'fp32' else bf16
    Pk = [p.cuda().requires_grad_(True) for p in P]
    x = x32.to(g_dt).cuda().requires_grad_(True)
    if form == 'res32':
        x._res32 = x32.cuda()
    D = x32.shape[1]
    ops.begin_step()
    out = ops.video_block(x, Pk, B, cfg.frames, cfg.n_patches, cfg.heads, D * cfg.mlp_ratio, cfg.eps_video,
                          dp_scale=None if dp is None else tuple(m.cuda() for m in dp))
    o = ops.stream32(out) if form == 'res32' else out
    out.backward(dout.cuda())
    torch.cuda.synchronize()
    return o.detach(), x.grad, [p.grad for p in Pk]


def _dp_ref(cfg, B, S, m_attn, m_mlp):
    def fn(sd, x):
        D = x.shape[-1]
        return dp_video_block(x.view(B, S, D), 0, sd, cfg, m_attn, m_mlp).reshape(B * S, D)
    return fn


@pytest.mark.gpu
@pytest.mark.parametrize('geom', ['small', 'ragged', 'base'])
@pytest.mark.parametrize('form', ['fp32', 'bf16', 'res32'])
def test_video_block_drop_path_vs_fp64_oracle(form, geom, monkeypatch):
    """ops.video_block(dp_scale=...) at B = 4 (every keep / drop combination) in fp32, bf16 with the bf16 stream and bf16 with the fp32
    stream: output and every gradient against the fp64 composition; multipliers all 1 bitwise equal to dp_scale=None; in fp32 a
    sample dropped on both branches leaves its input rows as they are, bit for bit."""
    from egovlpv2_amd import hipops as ops
    g, pc, cfg, sd = T._setup(geom)
    B, D = 4, g['dim']
    S = cfg.seq
    names = T.video_names(0, False)
    P = [sd[n] for n in names]
    monkeypatch.setenv('EGV_VIDEO_RES32', '0' if form == 'bf16' else '1')
    x32 = T._rnd((B * S, D), 41)
    x_in = x32 if form in ('fp32', 'res32') else x32.to(bf16).float()
    dout = T._rnd((B * S, D), 42).to(torch.float32 if form == 'fp32' else bf16)

    o, dx, dps = _run_block(ops, P, x32, form, B, cfg, dout, (M_ATTN, M_MLP))
    fn = _dp_ref(cfg, B, S, M_ATTN, M_MLP)
    (o64,), gi64, gp64, sc64 = T._oracle(fn, names, P, [x_in], [dout], torch.float64)
    oac = giac = gpac = None
    if form != 'fp32':
        (oac,), giac, gpac, _ = T._oracle(fn, names, P, [x_in], [dout], torch.float32, mixed=True)
    cls = lambda t: None if t is None else t.reshape(B, S, D)[:, 0]          # noqa: E731
    items = [('out', o, o64, oac, False), ('out[CLS]', cls(o), cls(o64), cls(oac), False),
             ('dx', dx, gi64[0], None if giac is None else giac[0], True),
             ('dx[CLS]', cls(dx), cls(gi64[0]), cls(None if giac is None else giac[0]), True)]
    items += T._items('d ', names, dps, gp64, gpac, sc64)
    T._compare(f'video drop path {form} {geom}', items, 'fp32' if form == 'fp32' else 'bf16')

    if form == 'fp32':                             # sample 3: both branches dropped -> out = x exactly
        assert torch.equal(o.reshape(B, S, D)[3].cpu(), x32.reshape(B, S, D)[3])
    ones = torch.ones(B)
    a = _run_block(ops, P, x32, form, B, cfg, dout, (ones, ones))
    b = _run_block(ops, P, x32, form, B, cfg, dout, None)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for n, ga, gb in zip(names, a[2], b[2]):
        assert torch.equal(ga, gb), n


@pytest.mark.gpu
@pytest.mark.parametrize('form', ['fp32', 'bf16', 'res32'])
def test_video_block_space_branch_dropped_everywhere_has_zero_gradients(form, monkeypatch):
    """every sample dropped on the space branch: what only reaches the output through it -- timeattn.*, attn.*, norm3, norm1 -- gets
    exactly zero gradient (not a rounding residue)"""
    from egovlpv2_amd import hipops as ops
    g, pc, cfg, sd = T._setup('small')
    B, D = 4, g['dim']
    names = T.video_names(0, False)
    P = [sd[n] for n in names]
    monkeypatch.setenv('EGV_VIDEO_RES32', '0' if form == 'bf16' else '1')
    x32 = T._rnd((B * cfg.seq, D), 51)
    dout = T._rnd((B * cfg.seq, D), 52).to(torch.float32 if form == 'fp32' else bf16)
    _, _, dps = _run_block(ops, P, x32, form, B, cfg, dout, (torch.zeros(B), M_MLP))
    for n, gp in zip(names, dps):
        if any(k in n for k in ('.timeattn.', '.attn.', '.norm3.', '.norm1.')):
            assert gp is not None and int(torch.count_nonzero(gp)) == 0, n
        elif n.endswith('.weight') and '.mlp.' in n:
            assert int(torch.count_nonzero(gp)) > 0, n


@pytest.mark.gpu
@pytest.mark.parametrize('geom', ['small', 'ragged'])
def test_video_layernorm_fold_chain_drop_path_vs_fp64_oracle(geom):
    """two fp32-stream blocks with drop path, the first folding the second's norm3 into its output pass (EGV_LN_FOLD,
    BLOCK_H3_READY): output, dx and both blocks' gradients against the fp64 chain"""
    from egovlpv2_amd import hipops as ops
    g, pc, cfg, sd = T._setup(geom)
    B, D = 4, g['dim']
    S, H, Hd, eps = cfg.seq, cfg.heads, D * cfg.mlp_ratio, cfg.eps_video
    n0, n1 = T.video_names(0, False), T.video_names(1, False)
    P0, P1 = [sd[n] for n in n0], [sd[n] for n in n1]
    m1a, m1m = M_MLP.flip(0), M_ATTN.flip(0)
    x32 = T._rnd((B * S, D), 61)
    dout = T._rnd((B * S, D), 62).to(bf16)

    ops.begin_step()
    K0, K1 = [p.cuda().requires_grad_(True) for p in P0], [p.cuda().requires_grad_(True) for p in P1]
    x = x32.to(bf16).cuda().requires_grad_(True)
    x._res32 = x32.cuda()
    mid = ops.video_block(x, K0, B, cfg.frames, cfg.n_patches, H, Hd, eps, next_ln=(K1[12], K1[13], 0, False),
                          dp_scale=(M_ATTN.cuda(), M_MLP.cuda()))
    assert '_pre_save' in mid.__dict__, 'the first block did not fold the next LayerNorm'
    out = ops.video_block(mid, K1, B, cfg.frames, cfg.n_patches, H, Hd, eps, dp_scale=(m1a.cuda(), m1m.cuda()))
    assert '_pre_save' not in mid.__dict__, 'the second block did not take the folded LayerNorm'
    o = ops.stream32(out)
    out.backward(dout.cuda())
    torch.cuda.synchronize()

    def chain(sd_, x_):
        v = dp_video_block(x_.view(B, S, D), 0, sd_, cfg, M_ATTN, M_MLP)
        return dp_video_block(v, 1, sd_, cfg, m1a, m1m).reshape(B * S, D)
    names, P = n0 + n1, P0 + P1
    (o64,), gi64, gp64, sc64 = T._oracle(chain, names, P, [x32], [dout], torch.float64)
    (oac,), giac, gpac, _ = T._oracle(chain, names, P, [x32], [dout], torch.float32, mixed=True)
    cls = lambda t: t.reshape(B, S, D)[:, 0]                                 # noqa: E731
    items = [('out', o, o64, oac, False), ('out[CLS]', cls(o), cls(o64), cls(oac), False),
             ('dx', x.grad, gi64[0], giac[0], True), ('dx[CLS]', cls(x.grad), cls(gi64[0]), cls(giac[0]), True)]
    items += T._items('d ', names, [p.grad for p in K0 + K1], gp64, gpac, sc64)
    T._compare(f'video drop path LayerNorm-fold chain {geom}', items, 'bf16')


@pytest.mark.gpu
def test_executor_refuses_drop_path_where_it_has_no_form():
    """the fused form (L > 0) and the CLS-only head call refuse dp_scale (an error, not ignored multipliers)"""
    from egovlpv2_amd import hipops as ops
    from egovlpv2_amd import _lib as L
    g, pc, cfg, sd = T._setup('small')
    B, Lt, D = 4, 8, g['dim']
    P = [sd[n].cuda() for n in T.video_names(1, True)]
    x = T._rnd((B * cfg.seq, D), 71).to(bf16).cuda()
    y = T._rnd((B * Lt, D), 72).to(bf16).cuda()
    m = torch.ones(B, device='cuda')
    with torch.no_grad(), pytest.raises(L.EgvError, match='drop path'):
        ops.video_block(x, P, B, cfg.frames, cfg.n_patches, cfg.heads, D * cfg.mlp_ratio, cfg.eps_video, y=y,
                        y_mask=torch.zeros(B, Lt, device='cuda'), L=Lt, dp_scale=(m, m))


@pytest.mark.gpu
def test_drop_path_scales_values_and_keep_fraction():
    from egovlpv2_amd import hipops as ops
    n, p = 1 << 20, 0.3
    keep = 1.0 - p
    m = ops.drop_path_scales(n, p, 0x1234ABCD).cpu()
    inv = torch.tensor(1.0 / keep, dtype=torch.float32)
    assert bool(((m == 0) | (m == inv)).all())
    frac = float((m != 0).double().mean())
    assert abs(frac - keep) <= 5 * math.sqrt(keep * p / n), frac
    assert torch.equal(ops.drop_path_scales(n, p, 0x1234ABCD).cpu(), m)
    assert not torch.equal(ops.drop_path_scales(n, p, 0x1234ABCE).cpu(), m)
    assert bool((ops.drop_path_scales(64, 0.0, 7).cpu() == 1).all())


# ---- GPU: model level (fine-tune variant, task Dual) ---------------------------------------------------------------------------------
def _ft_model(cfg, sd, dtype, rate):
    from egovlpv2_amd.model.model_epic_charades import FrozenInTime
    m = FrozenInTime({'model': 'SpaceTimeTransformer', 'num_frames': cfg.frames, 'pretrained': True, 'drop_path_rate': rate},
                     {'model': 'roberta-base', 'pretrained': True, 'input': 'text'}, path_config=cfg, compute_dtype=dtype)
    m.load_state_dict({k: v.detach() for k, v in sd.items()}, strict=True)
    m = m.cuda()
    m._drop_p = lambda: 0.0              # text-tower dropout off: the oracle has none, drop path is what is under test
    return m


def _step(m, dev, ds, seed=None):
    from egovlpv2_amd.model.loss import AdaptiveMaxMarginRankingLoss, NormSoftmaxLoss
    from egovlpv2_amd.trainer.trainer_egoclip import AllGather_multi
    fn = AdaptiveMaxMarginRankingLoss(margin=0.2) if ds == 'epic' else NormSoftmaxLoss()
    if seed is not None:
        m.seed_dropout(seed)
    m.zero_grad(set_to_none=True)
    loss, _, ret = m(dev, AllGather_multi.apply, 1, types.SimpleNamespace(world_size=1, rank=0), {}, fn, 0, task_names='Dual',
                     dataset_name=ds)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}


def _dev(data):
    return {'video': data['video'].cuda(), 'text': {k: v.cuda() for k, v in data['text'].items()}, 'relation': data['relation'].cuda()}


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['dual_tiny', 'dual_base_f4'])
@pytest.mark.parametrize('dtype,tol_l,tol_g', [(torch.float32, 1e-3, 5e-3), (torch.bfloat16, 2e-2, 0.15)])
def test_dual_finetune_drop_path_vs_oracle(name, dtype, tol_l, tol_g, monkeypatch):
    """train mode, drop_path_rate 0.2, both datasets: loss and the whole gradient against O.dual_forward_loss with the recorded
    multipliers applied in the oracle's blocks (tolerances of test_dual_finetune_variant_vs_golden)"""
    from egovlpv2_amd.synthetic import make_state_dict
    g, cfg, B, L, wseed, bseed = load_golden_dual(name)
    sd = make_state_dict(cfg, wseed, 'Dual')
    m = _ft_model(cfg, sd, dtype, 0.2).train()
    data = dual_batch(cfg, B, L, bseed)
    dev = _dev(data)
    oc = O.make_cfg(**cfg.as_dict())
    for v in sd.values():
        if v.is_floating_point():
            v.requires_grad_(True)
    for ds, seed in (('epic', 3), ('charades', 4)):
        loss, grads = _step(m, dev, ds, seed)
        rec = {i: (a.cpu(), b.cpu()) for i, (a, b) in m.last_drop_path_scales.items()}
        assert sorted(rec) == list(range(cfg.depth))
        assert all(bool((t == 1).all()) for t in rec[0])                     # block 0: rate 0
        print(f'\n[drop path] {name} {ds}: multipliers', {i: (a.tolist(), b.tolist()) for i, (a, b) in rec.items()})

        def block(x, i, sd_, cfg_, y=None, y_mask_add=None):
            assert y is None
            return dp_video_block(x, i, sd_, cfg_, rec[i][0].to(x.dtype), rec[i][1].to(x.dtype))
        monkeypatch.setattr(O, 'video_block', block)
        for v in sd.values():
            v.grad = None
        oloss, _, _, _ = O.dual_forward_loss(sd, data, oc, ds)
        oloss.backward()
        monkeypatch.undo()
        ref = float(oloss)
        assert abs(float(loss) - ref) <= tol_l * abs(ref) + (0 if dtype == torch.float32 else 2e-3), (ds, float(loss), ref)
        num = den = dot = gg = 0.0
        for k, p in m.named_parameters():
            if sd[k].grad is None:
                assert k not in grads or float(grads[k].abs().max()) == 0.0, k
                continue
            a, b = grads[k].double().cpu(), sd[k].grad.double()
            num += float((a - b).pow(2).sum()); den += float(b.pow(2).sum()); dot += float((a * b).sum()); gg += float(a.pow(2).sum())
        assert math.sqrt(num / den) < tol_g, (ds, math.sqrt(num / den))
        assert dot / math.sqrt(gg * den) > (0.999 if dtype == torch.float32 else 0.99), ds


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_dual_finetune_drop_path_determinism(dtype):
    """eval mode at rate 0.2 is bitwise rate 0; the same seed_dropout gives bitwise the same step, another seed other multipliers;
    activation checkpointing on and off give bitwise the same gradients"""
    from egovlpv2_amd.synthetic import make_state_dict
    g, cfg, B, L, wseed, bseed = load_golden_dual('dual_base_f4')
    sd = make_state_dict(cfg, wseed, 'Dual')
    dev = _dev(dual_batch(cfg, B, L, bseed))
    m = _ft_model(cfg, sd, dtype, 0.2)
    m0 = _ft_model(cfg, sd, dtype, 0.0)
    la, ga = _step(m.eval(), dev, 'charades', 1)
    lb, gb = _step(m0.eval(), dev, 'charades', 1)
    assert m.last_drop_path_scales == {}
    assert torch.equal(la, lb) and ga.keys() == gb.keys() and all(torch.equal(ga[k], gb[k]) for k in ga)

    m.train()
    l1, g1 = _step(m, dev, 'epic', 11)
    s1 = {i: (a.clone(), b.clone()) for i, (a, b) in m.last_drop_path_scales.items()}
    l2, g2 = _step(m, dev, 'epic', 11)
    s2 = m.last_drop_path_scales
    assert all(torch.equal(s1[i][j], s2[i][j]) for i in s1 for j in (0, 1))
    assert torch.equal(l1, l2) and all(torch.equal(g1[k], g2[k]) for k in g1)
    for seed in range(12, 20):                  # (a tiny batch can draw the same multipliers twice by chance: some other seed must not)
        _step(m, dev, 'epic', seed)
        s3 = m.last_drop_path_scales
        if any(not torch.equal(s1[i][j], s3[i][j]) for i in s1 if i > 0 for j in (0, 1)):
            break
    else:
        raise AssertionError('eight other seeds drew the multipliers of seed 11')

    mc = _ft_model(cfg, sd, dtype, 0.2).train()
    mc.act_checkpoint = True                      # (FrozenInTime(activation_checkpointing=True) of the pre-training constructor)
    lc, gc = _step(mc, dev, 'epic', 11)
    assert all(torch.equal(s1[i][j], mc.last_drop_path_scales[i][j]) for i in s1 for j in (0, 1))
    assert torch.equal(lc, l1) and gc.keys() == g1.keys() and all(torch.equal(gc[k], g1[k]) for k in g1)
