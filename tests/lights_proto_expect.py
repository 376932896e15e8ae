"""A plain numpy model of the A2C and GAT-DQN light protocols (include/trafficsim_lights_proto.h), written from
utilities/light_group_managment/rl_a2c.py:41-70, 135-163 and rl_gatdqn.py:105-173, 283-331 of the reference.

Inputs: the light tables of a trace / world dict, the occupancy map as an (H, W) array, the controller state
(tests/lights_ext_expect.Ctrl: _rl_phase, rl_timer, current, pending, repop) and the actions.  Everything is computed in
Python floats (doubles) and rounded to float32 once.  The epsilon-greedy draws are not modelled here: the fixtures record
the action taken, and the GPU replay proves the draws through the global stream's fingerprint."""
import numpy as np

from tests import lights_ext_expect as lx

A2C, GAT = 1, 2
ORDER = (0, 2, 1, 3)      # N, S, E, W as the direction codes of g_neighbors (N 0, E 1, S 2, W 3)


def a2c_state(tabs, occ, ctrl, static):
    size, pen = static
    s = lx.local_sums(tabs, occ)
    G = len(s)
    out = np.zeros((G, 13), dtype=np.float64)
    for g in range(G):
        nbrs = lx._neighbours(tabs, ctrl, g)
        cnt = max(1, len(nbrs))
        ns, ew = int(s[g, 0]), int(s[g, 1])
        bits = [1, 0] if ctrl.rl_phase[g] == 0 else [0, 1]
        # 4-5 and 11: getattr(n, '_pressure_ns' / '_pressure_ew' / 'intersection_size_factor', 0) - attributes nothing sets
        out[g] = [float(ns), float(ew), ns - ew, ew - ns, 0 / cnt, 0 / cnt] + bits + [int(ctrl.rl_timer[g]) / lx.TIMER_NORM] + \
                 [size[g], pen[g], 0 / cnt, sum(pen[n] for n in nbrs) / cnt]
    return out.astype(np.float32)


def _node(s, j, phase, t_norm, static):
    ns, ew = int(s[j, 0]), int(s[j, 1])
    return [float(ns), float(ew), float(ns - ew), float(ew - ns)] + ([1.0, 0.0] if phase == 0 else [0.0, 1.0]) + \
           [float(t_norm), float(static[0][j]), float(static[1][j])]


def _graph(tabs, s, g, ctrl, static, phase_of):
    nb = (tabs["g_neighbors"] if ctrl.repop[g] else tabs["g_neighbors_ctor"])[g]
    by_dir = {int(d): int(n) for d, n in nb if d >= 0 and n >= 0}
    feat = [_node(s, g, int(ctrl.rl_phase[g]), int(ctrl.rl_timer[g]) / lx.TIMER_NORM, static)]
    mask = [1.0]
    for d in ORDER:
        if d in by_dir:
            n = by_dir[d]
            feat.append(_node(s, n, phase_of(n), 0 / lx.TIMER_NORM, static))      # (`_rl_timer`: never set)
            mask.append(1.0)
        else:
            feat.append([0.0] * 9)
            mask.append(0.0)
    return feat, mask


def gat_state(tabs, occ, ctrl, static):
    s = lx.local_sums(tabs, occ)
    G = len(s)
    both = [_graph(tabs, s, g, ctrl, static, lambda n: int(ctrl.rl_phase[n])) for g in range(G)]
    return (np.asarray([b[0] for b in both], dtype=np.float64).reshape(G, 5, 9).astype(np.float32),
            np.asarray([b[1] for b in both], dtype=np.float64).reshape(G, 5).astype(np.float32))


def global_term(stats):
    """rl_gatdqn.py:314-318 on [avg_duration_internal, _through, avg_time_per_unit_internal, _through]"""
    avg_dur = 0.5 * (stats[0] + stats[1])
    avg_tpb = 0.5 * (stats[2] + stats[3])
    return 0.01 * avg_dur + 1.0 * avg_tpb


def act(tabs, occ, ctrl, actions, protocol, min_green=5, static=None, stats=(0.0, 0.0, 0.0, 0.0)):
    """The loop of rl_a2c.py:135-164 / rl_gatdqn.py:297-331 over the groups in table order.  Returns the rewards (float64),
    and under GAT the next states, each evaluated inside the loop."""
    s = lx.local_sums(tabs, occ)
    G = len(s)
    reward = np.zeros(G, dtype=np.float64)
    nxt = np.zeros((G, 5, 9), dtype=np.float64)
    for g in range(G):
        ctrl.rl_timer[g] += 1
        if ctrl.rl_timer[g] == 1:
            lx.apply_phase(ctrl, g, int(ctrl.rl_phase[g]))
        if int(actions[g]) == 1 and ctrl.rl_timer[g] >= min_green:
            ctrl.rl_phase[g] = 1 - ctrl.rl_phase[g]
            ctrl.rl_timer[g] = 0
        ns, ew = int(s[g, 0]), int(s[g, 1])
        if protocol == A2C:
            reward[g] = -float((ns + ew) + 0.25 * (ns - ew) ** 2)
        else:
            reward[g] = -(float(ns + ew) + float(global_term(stats)))
            nxt[g] = _graph(tabs, s, g, ctrl, static, lambda n: int(ctrl.rl_phase[n]))[0]      # (j < g moved already, j > g not yet)
    return (reward, nxt.astype(np.float32)) if protocol == GAT else reward


def epsilon_after(eps, eps_min, eps_decay):
    return np.asarray([max(eps_min, float(e) - eps_decay) for e in eps], dtype=np.float64)
