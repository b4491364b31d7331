"""CPU replica of the kernels' counter-hash dropout mask (csrc/common.h: hash_u32, dropout_scale) -- test infrastructure only,
imports nothing from the package.

The mask is a pure function of (rng[0], rng[1], stream_id, m * K + k, p):
    seed = rng[0] + 0x9E3779B9 * rng[1]                                 (csrc/heads.hip ColProlog, csrc/linear_big.hip Prolog)
    h    = hash_u32(idx * 0x9E3779B9 + hash_u32(seed ^ (stream_id * 0x85ebca6b)))
    u    = float32(h >> 8) * 2^-24;   dropped iff u < float32(p);   kept value float32(1) / (float32(1) - float32(p))
all in uint32 with wrap-around.  rng is the engine's int32 tensor [seed word, step counter]; stream_id is the index of the layer in
engine.head_program(model)["lins"] plus one."""
import numpy as np
import torch
import torch.nn as nn

GOLDEN = 0x9E3779B9
STREAM_MUL = 0x85EBCA6B
_M32 = 0xFFFFFFFF


def _u32(x):
    """int / int array (negative int32 values included) -> uint32 array, two's complement"""
    return (np.asarray(x, dtype=np.int64) & _M32).astype(np.uint32)


def hash_u32(x):
    """common.h hash_u32, vectorised over uint32"""
    x = np.array(x, dtype=np.uint32, copy=True)
    with np.errstate(over="ignore"):          # (numpy warns about wrap-around of 0-d operands only; wrap-around is the point)
        x ^= x >> np.uint32(16)
        x *= np.uint32(0x7FEB352D)
        x ^= x >> np.uint32(15)
        x *= np.uint32(0x846CA68B)
        x ^= x >> np.uint32(16)
    return x


def seed_of(rng0, counter):
    with np.errstate(over="ignore"):
        return _u32(rng0) + np.uint32(GOLDEN) * _u32(counter)


def uniform(seed, stream_id, idx):
    """the kernels' u of (seed, stream, element index), float32 in [0, 1)"""
    with np.errstate(over="ignore"):
        inner = hash_u32(_u32(seed) ^ (_u32(stream_id) * np.uint32(STREAM_MUL)))
        h = hash_u32(_u32(idx) * np.uint32(GOLDEN) + inner)
    return (h >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def mask(rng0, counter, stream_id, M, K, p):
    """-> float32 [M, K] multiplicative mask of one layer's input: 0 (dropped) or 1 / (1 - p) (kept)"""
    with np.errstate(over="ignore"):
        u = uniform(seed_of(rng0, counter), stream_id, np.arange(M * K, dtype=np.int64))
    p32 = np.float32(p)
    keep = np.float32(1.0) / (np.float32(1.0) - p32)
    return np.where(u < p32, np.float32(0.0), keep).astype(np.float32).reshape(M, K)


# ---- scalar restatement in plain Python ints (the check of the vectorised form, tests/test_cpu_dropout_ref.py) -------------------
def hash_u32_int(x):
    x &= _M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & _M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & _M32
    x ^= x >> 16
    return x


def scale_int(rng0, counter, stream_id, idx, p):
    seed = ((rng0 & _M32) + GOLDEN * (counter & _M32)) & _M32
    inner = hash_u32_int(seed ^ ((stream_id * STREAM_MUL) & _M32))
    h = hash_u32_int((((idx & _M32) * GOLDEN) & _M32) + inner)
    u = np.float32(h >> 8) * np.float32(2.0 ** -24)
    p32 = np.float32(p)
    return np.float32(0.0) if u < p32 else np.float32(1.0) / (np.float32(1.0) - p32)


# ---- oracle side: nn.Dropout replaced by "multiply by the given tensor; identity in eval" --------------------------------------
class MaskedDropout(nn.Module):
    def __init__(self, p):
        super().__init__()
        self.p = p
        self.mask = None          # [B, K] tensor, set per step (ReplicaDropout.set); None = identity

    def forward(self, x):
        if not self.training or self.mask is None:
            return x
        assert tuple(self.mask.shape) == tuple(x.shape), (tuple(self.mask.shape), tuple(x.shape))
        return x * self.mask.to(x.dtype)


def _set_module(root, name, new):
    parts = name.split(".")
    for q in parts[:-1]:
        root = getattr(root, q)
    setattr(root, parts[-1], new)


class ReplicaDropout(nn.Module):
    """An oracle model whose nn.Dropout modules multiply by the replica's masks.  The module -> stream map is read from the HIP side's
    head program (`lins`: engine.head_program(hip_model)["lins"]): entry i with pro_drop gives stream i + 1 and K = lin.in_features;
    the HIP model's and the oracle's Dropout modules are matched by module name.  Every Dropout of the oracle with p > 0 must be mapped
    (a layer the program forgot fails here, not silently)."""

    def __init__(self, oracle, hip_model, lins):
        super().__init__()
        hip_names = {id(m): n for n, m in hip_model.named_modules()}
        self.streams = {}                                    # module name -> (stream id, K, p)
        for i, L in enumerate(lins):
            if L.pro_drop is not None:
                self.streams[hip_names[id(L.pro_drop)]] = (i + 1, int(L.lin.in_features), float(L.pro_drop.p))
        self.drops = {}
        for name, m in list(oracle.named_modules()):
            if isinstance(m, nn.Dropout):
                if name not in self.streams:
                    assert m.p == 0.0, "oracle Dropout %s (p = %g) has no stream in the head program" % (name, m.p)
                    continue
                assert abs(m.p - self.streams[name][2]) < 1e-12, (name, m.p, self.streams[name][2])
                new = MaskedDropout(m.p)
                _set_module(oracle, name, new)
                self.drops[name] = new
        assert set(self.drops) == set(self.streams), (sorted(self.drops), sorted(self.streams))
        self.model = oracle

    def set(self, rng0, counter, B):
        """masks of the step with counter value `counter` on a batch of B rows (None: no masks = dropout off)"""
        for name, d in self.drops.items():
            if counter is None:
                d.mask = None
            else:
                s, K, p = self.streams[name]
                d.mask = torch.from_numpy(mask(rng0, counter, s, B, K, p))
        return self

    def forward(self, *args):
        return self.model(*args)
