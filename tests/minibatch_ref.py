"""Reference of the shuffled PPO minibatches (PPO minibatch="shuffled"), written from the definition in
include/flyhip.h in numpy uint32 and sharing nothing with the kernel: the keyed permutation, the gather, the rank-seed rule and
the epoch key."""
import numpy as np

GOLDEN = 0x9E3779B9
M32 = 0xFFFFFFFF


def lowbias32(x):
    x = np.asarray(x, dtype=np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7FEB352D)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846CA68B)
    x ^= x >> np.uint32(16)
    return x


def perm_index(R, seed, epoch_key, positions):
    """pi(i) for every i of `positions` (each in [0, R)): a balanced 6-round Feistel network on [0, 2^b) with cycle walking."""
    R = int(R)
    assert 1 <= R < 2 ** 31
    pos = np.asarray(positions, dtype=np.int64).reshape(-1)
    assert pos.size == 0 or (pos.min() >= 0 and pos.max() < R)
    b = max(2, (R - 1).bit_length())
    b += b & 1
    h = np.uint32(b // 2)
    mask = np.uint32((1 << (b // 2)) - 1)
    with np.errstate(over="ignore"):
        key = lowbias32(np.uint32(int(seed) & M32) ^ lowbias32(np.uint32(int(epoch_key) & M32)))
        x = pos.astype(np.uint32)
        todo = np.ones(x.shape, dtype=bool)
        while todo.any():
            cur = x[todo]
            L, Q = cur >> h, cur & mask
            for r in range(6):
                f = lowbias32(Q + key + np.uint32((GOLDEN * (r + 1)) & M32)) & mask
                L, Q = Q, L ^ f
            cur = (L << h) | Q
            x[todo] = cur
            todo[todo] = cur >= np.uint32(R)
    return x.astype(np.int64)


def gather_ref(obs, act, logp, adv, target, seed, epoch_key, first, n):
    """The five gathered arrays and the indices: row k is source row pi(first + k).  Arrays are moved as int32 words, so every
    bit pattern survives."""
    R = obs.shape[0]
    idx = perm_index(R, seed, epoch_key, np.arange(first, first + n))
    words = [np.ascontiguousarray(a).view(np.int32)[idx] for a in (obs, act, logp, adv, target)]
    return words, idx


def rank_seed(seed, rank):
    """The seed rank `rank` uses: seed + rank * 0x9E3779B9, wrapping as uint32 (as domain randomisation)."""
    return (int(seed) + int(rank) * GOLDEN) & M32


def epoch_key(update, epochs, epoch):
    """The key of epoch `epoch` of update number `update` (counted from 0): (update * epochs + epoch) mod 2^32."""
    return (int(update) * int(epochs) + int(epoch)) & M32


def chunk_chi_square(R, n, seed, key):
    """For each of the R / n windows of n positions, the chi-square statistic of its rows' source chunks pi // n against the
    uniform expectation n / (R / n) per chunk."""
    chunks = R // n
    pi = perm_index(R, seed, key, np.arange(R))
    out = []
    for w in range(chunks):
        counts = np.bincount(pi[w * n:(w + 1) * n] // n, minlength=chunks).astype(np.float64)
        expect = n / chunks
        out.append(float(((counts - expect) ** 2 / expect).sum()))
    return out
