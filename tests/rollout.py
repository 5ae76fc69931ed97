"""Helpers of the rollout-buffer tests (include/smarties_hip_rollout.h): the noise mapping restated in numpy, a second restatement of the
Philox core in plain integers, the hand-written loop over the existing device calls that hl_rollout_step replaces, and a toy simulator."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57      # Philox4x32 multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85      # Weyl constants: golden ratio, sqrt(3) - 1
KAT_ZERO = (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)      # Random123's known answer: philox4x32-10, counter 0, key 0
KAT_ONES = (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)      # ... counter ffffffff x 4, key ffffffff x 2
NORMDIST_MAX = 3.0


def philox_np(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on arrays (uint64 arithmetic on 32-bit words); returns the four output words as uint64 arrays"""
    c = [np.asarray(x, dtype=np.uint64) & np.uint64(0xFFFFFFFF) for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = np.uint64(k0 & 0xFFFFFFFF), np.uint64(k1 & 0xFFFFFFFF)
    mask, sh = np.uint64(0xFFFFFFFF), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> sh) ^ c[1] ^ k0, p1 & mask, (p0 >> sh) ^ c[3] ^ k1, p0 & mask]
        k0, k1 = (k0 + np.uint64(W0)) & mask, (k1 + np.uint64(W1)) & mask
    return c


def philox_int(counter, key):
    """the same ten rounds in Python integers, written from the round function alone: (hi, lo) of two products, crossed over"""
    c, k = list(counter), list(key)
    for r in range(10):
        if r:
            k = [(k[0] + W0) % 2**32, (k[1] + W1) % 2**32]
        hi0, lo0 = divmod(M0 * c[0], 2**32)
        hi1, lo1 = divmod(M1 * c[2], 2**32)
        c = [hi1 ^ c[1] ^ k[0], lo1, hi0 ^ c[3] ^ k[1], lo0]
    return tuple(c)


def u53(hi, lo):
    return ((hi >> np.uint64(5)) * np.uint64(1 << 26) + (lo >> np.uint64(6))).astype(np.float64) * 2.0**-53


def noise_np(seed, env, episode, t, component, discrete=False, replaced=None):
    """the library's draw for (seed, env, episode, t, component), arrays broadcast against each other.  replaced: a list that receives
    the mask of the normal draws that fell beyond +-3"""
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    env, episode, t, component = np.broadcast_arrays(*[np.asarray(x, dtype=np.uint64) for x in (env, episode, t, component)])
    x = philox_np(env, episode, t, component, k0, k1)
    u1 = u53(x[0], x[1])
    if discrete:
        return u1
    u2 = u53(x[2], x[3])
    z = np.sqrt(-2.0 * np.log(1.0 - u1)) * np.cos((2.0 * np.pi) * u2)
    out = np.abs(z) > NORMDIST_MAX
    y = philox_np(env, episode, t, component + np.uint64(65536), k0, k1)
    if replaced is not None:
        replaced.append(out)
    return np.where(out, (2.0 * u53(y[0], y[1]) - 1.0) * NORMDIST_MAX, z)


# ---- the loop written by hand over the existing calls, tensors laid out as the slabs are ------------------------------------------------
class HandLoop:
    """What a user of hl_select_actions_sequences_dev and hl_append_episodes_dev keeps: slabs [nEnv maxSteps] rows, lengths in torch, the
    scatter and the terminal rows in torch, the ended environments found on the host in ascending order, tags tag_base + k."""

    def __init__(self, L, n_env, max_steps, tag_base=0):
        import torch
        self.L, self.n, self.T, self.tag_base, self.k = L, n_env, max_steps, tag_base, 0
        dev, rows = "cuda", n_env * max_steps
        self.S = torch.zeros((rows, L.dS), dtype=torch.float32, device=dev)
        self.A = torch.zeros((rows, L.dA), dtype=torch.float64, device=dev)
        self.MU = torch.zeros((rows, L.polDim), dtype=torch.float64, device=dev)
        self.R = torch.zeros(rows, dtype=torch.float64, device=dev)
        self.V = torch.zeros(rows, dtype=torch.float32, device=dev)
        self.ADV = torch.zeros(rows, dtype=torch.float32, device=dev)
        self.len = torch.zeros(n_env, dtype=torch.int64, device=dev)
        self.first = torch.arange(n_env, dtype=torch.int64, device=dev) * max_steps
        self.capped = 0

    def step(self, states, rewards, end, noise=None, store=True):
        import torch
        L, T = self.L, self.T
        t = self.len
        row = self.first + t
        self.S[row] = states
        self.R[row] = torch.where(t == 0, torch.zeros_like(rewards), rewards)
        ns = t + 1
        kind = torch.where(end == 1, 1, torch.where(end != 0, 2, 0))
        kind = torch.where((kind == 0) & (ns >= T), 3, kind)      # the cap closes the episode as truncated
        act, mu, v, adv = L.select_actions_sequences_dev(self.S, self.first, ns.int(), 1, noise)
        run = kind == 0
        out = torch.where(run[:, None], act, torch.zeros_like(act))
        self.A[row] = out
        self.MU[row] = torch.where(run[:, None], mu, torch.zeros_like(mu))
        self.V[row] = torch.where(kind == 1, torch.zeros_like(v), v)
        self.ADV[row] = torch.where(run, adv, torch.zeros_like(adv))
        self.len = torch.where(run, ns, torch.zeros_like(ns))
        kind_h, ns_h = torch.stack((kind, ns)).cpu().numpy()      # the host has to know which environments ended
        self.capped += int((kind_h == 3).sum())
        ended = np.flatnonzero((kind_h != 0) & (ns_h >= 2))       # ascending environment order
        if ended.size and store:
            L.append_episodes_dev(ns_h[ended], kind_h[ended] == 1, self.tag_base + self.k + np.arange(ended.size), ended * T, 1,
                                  self.S, self.A, self.MU, self.R, self.V, self.ADV)
            self.k += int(ended.size)
        return out

    def slab(self, env):
        T = self.T
        return [x[env * T:(env + 1) * T].cpu().numpy() for x in (self.S, self.A, self.MU, self.R, self.V, self.ADV)]


class ToySim:
    """a linear map on the device as the simulator; the end flags come from a fixed table of episode lengths per environment
    (0: never flagged)"""

    def __init__(self, n_env, dS, dA, lengths, seed=9, discrete=False):
        import torch
        rng = np.random.default_rng(seed)
        self.M = torch.from_numpy((rng.normal(size=(dS, dS)) * (0.4 / np.sqrt(dS / 6.0))).astype(np.float32)).cuda()
        self.K = torch.from_numpy((rng.normal(size=(dA, dS)) * 0.3).astype(np.float32)).cuda()
        self.s0 = torch.from_numpy(rng.normal(size=(n_env, dS)).astype(np.float32)).cuda()
        self.lengths = lengths      # per environment: a list of (states, end flag) gone round
        self.n = n_env
        self.reset()

    def reset(self):
        import torch
        self.s = self.s0.clone()
        self.r = torch.zeros(self.n, dtype=torch.float64, device="cuda")
        self.t = [0] * self.n
        self.ep = [0] * self.n

    def observe(self, max_steps):
        """(states, rewards, end flags, per environment whether the state ends its episode by its flag or by the cap) of the current step"""
        import torch
        end = []
        for e in range(self.n):
            table = self.lengths[e]
            n_states, flag = table[self.ep[e] % len(table)]
            end.append(flag if n_states and self.t[e] + 1 == n_states else 0)
        ended = [end[e] != 0 or self.t[e] + 1 >= max_steps for e in range(self.n)]
        return self.s, self.r, torch.tensor(end, dtype=torch.int32, device="cuda"), ended

    def advance(self, actions, ended):
        """apply the actions; `ended`: per environment, whether its state ended the episode (flag or cap): it restarts"""
        import torch
        nxt = torch.tanh(self.s @ self.M + actions.float() @ self.K)
        self.r = -(nxt.double() ** 2).sum(dim=1)
        mask = torch.tensor(ended, dtype=torch.bool, device="cuda")
        self.s = torch.where(mask[:, None], self.s0 + 0.01 * nxt, nxt)
        for e in range(self.n):
            if ended[e]:
                self.t[e] = 0
                self.ep[e] += 1
            else:
                self.t[e] += 1
