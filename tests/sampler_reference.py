"""The device sampler (gh_sample_id, csrc/common.h) restated in vectorised numpy: what the float32 engine's own draws are
pinned to (test_hip_device_sampler.py).  TEST INFRASTRUCTURE ONLY.

The rule: the t-th sampled edge of an iteration is the t-th value of a keyed permutation of [0, E) -- a 4-round Feistel
network on ceil(log2 E) bits (at least one), the halves modified alternately, cycle walking until the value is below E --
keyed by (seed, iteration), both taken modulo 2^64.

f64_reference.sample_ids states the same rule in Python integers only, one id at a time; it is this module's anchor
(test_sampler_reference_cpu.py compares the two on a grid) and stays as it is.  Here all S walks advance together in
uint64 arrays, whose products and sums wrap modulo 2^64 as the kernel's do, so a stream of thousands of iterations is
affordable on the CPU.
"""
import numpy as np

_M64 = (1 << 64) - 1
_U = np.uint64

# the grid on which the two restatements are compared (test_sampler_reference_cpu.py, test_f64_reference_cpu.py)
GRID_E = (1, 2, 3, 5, 33, 1000, 4096, 4097, 16384, 16385, 131072, (1 << 20) + 1)
GRID_SEEDS = (0, 1, 12345, 1 << 32, (1 << 63) + 5, (1 << 64) - 1)
GRID_ITERATIONS = (0, 1, 7, (1 << 32) + 3)
GRID_FULL_MAX_E = 16385      # full permutations (S = E) are checked up to here


def _mix32(x):
    """gh_mix32: the 64-bit finaliser, low 32 bits; x a uint64 array."""
    x = x ^ (x >> _U(33))
    x = x * _U(0xff51afd7ed558ccd)
    x = x ^ (x >> _U(33))
    x = x * _U(0xc4ceb9fe1a85ec53)
    x = x ^ (x >> _U(33))
    return x & _U(0xFFFFFFFF)


def key_of(seed, iteration):
    """The 64-bit key of (seed, iteration), as a Python int."""
    return ((int(seed) & _M64) * 0x9E3779B97F4A7C15 + (int(iteration) & _M64) * 0xD1B54A32D192ED03 + 0x2545F4914F6CDD1D) & _M64


def sample_ids(E, S, seed, iteration):
    """int32[S]: gh_sample_id(E, seed, iteration, t) for t = 0 .. S - 1 (S <= E)."""
    E, S = int(E), int(S)
    if not 0 <= S <= E:
        raise ValueError(f"need 0 <= S <= E, got S = {S}, E = {E}")
    bits = 1
    while (1 << bits) < E:
        bits += 1
    lb = bits // 2
    hb = bits - lb
    lmask, hmask, lsh = _U((1 << lb) - 1), _U((1 << hb) - 1), _U(lb)
    key = key_of(seed, iteration)
    rkey = [_U((key + (rnd << 56)) & _M64) for rnd in range(4)]
    out = np.arange(S, dtype=np.uint64)
    walking = np.arange(S)                      # positions of out still at or above E (all, before the first pass)
    while len(walking):
        x = out[walking]
        lo, hi = x & lmask, (x >> lsh) & hmask
        for rnd in range(4):
            if rnd % 2 == 0:
                hi = (hi ^ _mix32(rkey[rnd] + lo)) & hmask
            else:
                lo = (lo ^ _mix32(rkey[rnd] + hi)) & lmask
        x = (hi << lsh) | lo
        out[walking] = x
        walking = walking[x >= _U(E)]
    return out.astype(np.int32)


def stream(E, S, seed, first_iteration, T):
    """int32[T, S]: the ids of iterations first_iteration .. first_iteration + T - 1."""
    out = np.empty((int(T), int(S)), dtype=np.int32)
    for t in range(int(T)):
        out[t] = sample_ids(E, S, seed, int(first_iteration) + t)
    return out
