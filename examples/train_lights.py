"""A policy-gradient loop on the engine's light groups: `python examples/train_lights.py --size 96 --seed 3 --ticks 200`.

An illustration of the external light control (include/trafficsim_lights_ext.h), not a result: one small shared policy,
REINFORCE with a mean baseline, one update per tick.  The state vectors are torch tensors over the engine's own memory
(`lights_device()`), the actions are sampled on the device and handed over as a device tensor, and the reward is built
from the next tick's state vector (the reference's own reward is identically 0) - nothing inside the loop is copied to
the host.  torch is imported before the engine library is loaded, so that both share one HIP runtime."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from run_city import TRAFFIC  # noqa: E402


def run(size=96, seed=3, ticks=200, dim=13, hidden=32, lr=3e-3, every=50, out=print):
    from trafficsimulation_amd.mesa_api import CityModel
    torch.cuda.init()
    m = CityModel(size, size, seed=seed, traffic=dict(TRAFFIC, P_int=40000, P_thr=10000),
                  defaults={"TRAFFIC_LIGHT_AGENT_ALGORITHM": "EXTERNAL", "SRL_INPUT_DIMENSIONS": dim, "RAIN_ENABLED": False})
    eng = m.engine
    dev = eng.lights_device()
    state = dev["state"]                       # (G, dim) float32, rewritten in place by every observe
    torch.manual_seed(seed)
    policy = torch.nn.Sequential(torch.nn.Linear(dim, hidden), torch.nn.Tanh(), torch.nn.Linear(hidden, 2)).to(state.device)
    opt = torch.optim.Adam(policy.parameters(), lr=lr)
    log_prob = None
    queue_sum = torch.zeros((), device=state.device)
    history = []
    for t in range(1, ticks + 1):
        eng.lights_observe(to_host=False)
        s = state.clone()
        queue = s[:, 0] + s[:, 1]              # vehicles on the approach cells of every group
        if log_prob is not None:               # the last actions are judged by the queues they led to
            reward = -queue
            loss = -(log_prob * (reward - reward.mean())).mean()
            opt.zero_grad()
            loss.backward()
            opt.step()
        dist = torch.distributions.Categorical(logits=policy(s))
        action = dist.sample()
        log_prob = dist.log_prob(action)
        eng.lights_act(action.to(torch.int8), want_next=False)
        m.step()
        queue_sum += queue.sum()
        if t % every == 0 or t == ticks:
            history.append(float(queue_sum) / every)       # (the only read-back, once per report)
            out(f"tick {t:5d}  live {len(m.active_vehicle_agents):5d}  mean queued vehicles per tick {history[-1]:.1f}")
            queue_sum.zero_()
    return m, history


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=96)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--dim", type=int, default=13, choices=[7, 11, 13, 17, 19])
    ap.add_argument("--every", type=int, default=50)
    a = ap.parse_args()
    model, _ = run(a.size, a.seed, a.ticks, a.dim, every=a.every)
    model.close()
    print("TRAIN_OK")
