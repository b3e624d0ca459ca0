"""Cost of stochastic depth in the fine-tune variant's training step (model_epic_charades.py, task Dual, EPIC-Kitchens MIR loss):
drop_path_rate 0 against RATE (default 0.1) on ONE model whose per-block rates are switched between rounds, alternating A / B so
that clock and thermal drift fall on both.  Shape of configs/ft/epic.json: B = 16 clips of 16 x 224^2, bf16, 32 text tokens.
python tools/drop_path_step.py [--rate 0.1] [--rounds 8] [--steps 5] [--batch 16]
Prints one JSON line: median / min / max ms per step of each arm over the rounds, and the median difference."""
import argparse
import json
import os
import statistics
import sys
import time
import types

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from egovlpv2_amd import hipops as ops  # noqa: E402
from egovlpv2_amd.config import PathConfig  # noqa: E402
from egovlpv2_amd.synthetic import make_state_dict, make_batch, make_relation  # noqa: E402
from egovlpv2_amd.model.model_epic_charades import FrozenInTime  # noqa: E402
from egovlpv2_amd.model.loss import AdaptiveMaxMarginRankingLoss  # noqa: E402
from egovlpv2_amd.trainer.trainer_egoclip import AllGather_multi  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--rate', type=float, default=0.1)
ap.add_argument('--rounds', type=int, default=8)
ap.add_argument('--steps', type=int, default=5)
ap.add_argument('--batch', type=int, default=16)
ap.add_argument('--text-len', type=int, default=32)
a = ap.parse_args()

dev = torch.device('cuda', 0)
cfg = PathConfig(frames=16, proj_dim=256, proj_style='linear', drop_rate=0.1)
model = FrozenInTime({'model': 'SpaceTimeTransformer', 'num_frames': cfg.frames, 'pretrained': True, 'drop_path_rate': a.rate},
                     {'model': 'roberta-base', 'pretrained': True, 'input': 'text'}, path_config=cfg, compute_dtype=torch.bfloat16)
model.load_state_dict(make_state_dict(cfg, 0, 'Dual'), strict=True)
model = model.to(dev).train()
rates = {0.0: None, a.rate: model._dp_rates}
data, _, _ = make_batch(cfg, a.batch, a.text_len, 1234)
data = {'video': data['video'].to(dev), 'text': {k: v.to(dev) for k, v in data['text'].items()},
        'relation': make_relation(a.batch, 1234).to(dev)}
args = types.SimpleNamespace(world_size=1, rank=0)
loss_fn = AdaptiveMaxMarginRankingLoss(margin=0.2)


def step():
    ops.invalidate_weight_cache()
    for p in model.parameters():
        p.grad = None
    loss, _, _ = model(data, AllGather_multi.apply, 1, args, {}, loss_fn, 0, task_names='Dual', dataset_name='epic')
    loss.backward()


def timed(rate):
    model._dp_rates = rates[rate]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / a.steps


for r in rates:                     # warm-up of both arms (allocator, weight copies, kernels of the drop-path form)
    model._dp_rates = rates[r]
    for _ in range(3):
        step()
res = {r: [] for r in rates}
for i in range(a.rounds):
    for r in (list(rates) if i % 2 == 0 else list(rates)[::-1]):
        res[r].append(timed(r))
arm = {f'rate_{r:g}': {'median_ms': statistics.median(v), 'min_ms': min(v), 'max_ms': max(v)} for r, v in res.items()}
diff = [b - z for z, b in zip(res[0.0], res[a.rate])]
print(json.dumps({'metric': 'finetune_dual_step_drop_path', 'batch': a.batch, 'frames': cfg.frames, 'rounds': a.rounds, 'steps': a.steps,
                  **arm, 'median_delta_ms': statistics.median(diff), 'delta_min_ms': min(diff), 'delta_max_ms': max(diff)}))
