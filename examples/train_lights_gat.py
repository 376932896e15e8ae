#!/usr/bin/env python3
"""A masked-attention Q-network on the engine's GAT-DQN environment (include/trafficsim_lights_proto.h), in torch on the
device tensors: with to_host=False state, mask, actions, reward and next state stay on the GPU (the engine's epsilon-greedy
step, which picks the actions, brings one greedy byte per group to the host and sends one action byte back).

An illustration of the interface, not a result: one shared network for all groups, one-step TD on the transitions of the
current tick only (no replay memory, no target network).

    python examples/train_lights_gat.py [ticks]
"""
import os
import sys

import torch  # before the engine library is loaded: it then shares torch's HIP runtime

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from run_city import TRAFFIC  # noqa: E402
from trafficsimulation_amd.mesa_api import CityModel  # noqa: E402


class StarAttentionQ(torch.nn.Module):
    """Single-head attention of the centre node over itself and its (masked) neighbours, then a small MLP to two q-values."""

    def __init__(self, features=9, width=16, hidden=32):
        super().__init__()
        self.w = torch.nn.Linear(features, width, bias=False)
        self.a = torch.nn.Linear(2 * width, 1, bias=False)
        self.head = torch.nn.Sequential(torch.nn.Linear(width, hidden), torch.nn.ReLU(), torch.nn.Linear(hidden, 2))

    def forward(self, feat, mask):
        h = self.w(feat)                                               # (G, 5, width)
        centre = h[:, :1].expand_as(h)
        e = torch.nn.functional.leaky_relu(self.a(torch.cat([centre, h], dim=-1)).squeeze(-1), 0.2)
        alpha = torch.softmax(e.masked_fill(mask == 0, -1e9), dim=1)   # absent directions get no weight
        return self.head(torch.relu((alpha.unsqueeze(-1) * h).sum(dim=1)))


def main(ticks=200):
    torch.cuda.init()
    model = CityModel(128, 128, seed=7, traffic=dict(TRAFFIC, P_int=40000, P_thr=10000),
                      defaults={"TRAFFIC_LIGHT_AGENT_ALGORITHM": "GAT_DQN_BATCHED", "RAIN_ENABLED": False, "EPS_DECAY_RATE": 0.01})
    dev = model.engine.lights_proto_device()
    net = StarAttentionQ().to(dev["state"].device)
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    for t in range(ticks):
        model.light_states(to_host=False)                              # fills dev["state"] / dev["mask"], nothing comes down
        state, mask = dev["state"].clone(), dev["mask"].clone()
        q = net(state, mask)
        model.control_lights_q(q.detach().contiguous(), to_host=False)  # epsilon-greedy on the engine's global stream
        action = dev["actions"].long()
        with torch.no_grad():
            target = dev["reward"].float() + 0.99 * net(dev["next_state"], mask).max(dim=1).values
        loss = torch.nn.functional.mse_loss(q.gather(1, action[:, None]).squeeze(1), target)
        opt.zero_grad()
        loss.backward()
        opt.step()
        model.step()
        if t % 20 == 0:
            print(f"tick {t}: loss {loss.item():.3f}  mean reward {dev['reward'].mean().item():.2f}  "
                  f"epsilon {model.intersection_light_groups[0].epsilon:.2f}")
    model.close()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 200)
