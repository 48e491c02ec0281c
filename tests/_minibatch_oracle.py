"""Host restatement of ``MinibatchRegressionModel`` (VB_MODEL_MINIBATCH_GLM): TEST INFRASTRUCTURE ONLY.

The batch indices are written again from the definition in DESIGN.md 4.23, with plain Python ints over the Philox4x32-10 of
``tests/_philox_oracle.py`` -- not from the package's vectorised restatement, and not from the device code:

* batch ``t`` owns the stream positions ``q = t B .. t B + B - 1``; position ``q`` is slot ``q mod n_data`` of epoch
  ``q div n_data``;
* ``order='sequential'``: the observation is the slot;
* ``order='shuffle'``: the observation is ``perm_epoch(slot)``, a balanced Feistel network on ``2 w`` bits,
  ``w = max(1, ceil(ceil(log2 n_data) / 2))``, cycle-walked into ``[0, n_data)``::

      x = slot
      repeat:  L, R = x >> w, x & (2^w - 1)
               for r in 0 .. 5:  L, R = R, L ^ F(r, R)
               x = (L << w) | R
      until x < n_data
      F(r, h) = word 0 of philox4x32_10(counter = (h, r, epoch mod 2^32, epoch div 2^32),
                                        key = (seed mod 2^32, seed div 2^32))  &  (2^w - 1)

The density of batch ``t`` on ``X[idx]``, with the interface of ``oracle/models.py`` (``logp``, ``grad``) plus ``pointwise``::

    f_t(theta) = (n_data / B) sum_{j in idx} l(y_j, x_j' theta) - |theta|^2 / (2 sd^2) - p (log sd + log(2 pi) / 2) + C
    l: the term WITHOUT the likelihood's constant; C: that constant summed over ALL n_data observations
    pointwise: l + the observation's own constant, unscaled
"""
import math

import numpy as np

import _philox_oracle as P
from _sparse_oracle import LOG_2PI, terms

ROUNDS = 6


def half_bits(n_data):
    bits = 0
    while (1 << bits) < n_data:            # ceil(log2 n_data)
        bits += 1
    return max(1, -(-bits // 2))


def round_function(r, h, epoch, seed, w):
    word0 = P.philox4x32_10(h, r, epoch & 0xFFFFFFFF, epoch >> 32, seed & 0xFFFFFFFF, seed >> 32)[0]
    return int(word0) & ((1 << w) - 1)


def permute(slot, epoch, n_data, seed):
    """perm_epoch(slot), and the number of Feistel passes the cycle walk took."""
    w = half_bits(n_data)
    x, walks = int(slot), 0
    while True:
        left, right = x >> w, x & ((1 << w) - 1)
        for r in range(ROUNDS):
            left, right = right, left ^ round_function(r, right, epoch, seed, w)
        x, walks = (left << w) | right, walks + 1
        if x < n_data:
            return x, walks


def permute_array(slots, epochs, n_data, seed):
    """``permute`` for arrays of slots and epochs (broadcast against each other) in one pass per Feistel round: the same
    definition on uint64 arrays, for the tests that need tens of thousands of epochs.  tests/test_minibatch_cpu.py checks it
    against ``permute`` element by element."""
    w = half_bits(n_data)
    ws, mask = np.uint64(w), np.uint64((1 << w) - 1)
    slots, epochs = np.broadcast_arrays(np.asarray(slots, dtype=np.uint64), np.asarray(epochs, dtype=np.uint64))
    x, epochs = slots.ravel().copy(), epochs.ravel()
    todo = np.arange(x.size)
    while todo.size:
        e = epochs[todo]
        left, right = x[todo] >> ws, x[todo] & mask
        for r in range(ROUNDS):
            word0 = P.philox4x32_10(right, r, e & np.uint64(0xFFFFFFFF), e >> np.uint64(32), seed & 0xFFFFFFFF, seed >> 32)[0]
            left, right = right, left ^ (word0 & mask)
        x[todo] = (left << ws) | right
        todo = todo[x[todo] >= np.uint64(n_data)]
    return x.astype(np.int64).reshape(slots.shape)


def batch_indices(t, n_data, batch_size, seed, order='shuffle'):
    out = np.empty(batch_size, dtype=np.int64)
    for i in range(batch_size):
        q = t * batch_size + i
        slot, epoch = q % n_data, q // n_data
        out[i] = slot if order == 'sequential' else permute(slot, epoch, n_data, seed)[0]
    return out


def batch_indices_array(t, n_data, batch_size, seed, order='shuffle'):
    """``batch_indices`` through ``permute_array`` (for batches of thousands)."""
    q = [t * batch_size + i for i in range(batch_size)]
    slots = np.array([v % n_data for v in q], dtype=np.int64)
    if order == 'sequential':
        return slots
    return permute_array(slots, np.array([v // n_data for v in q], dtype=np.uint64), n_data, seed)


def epoch_permutation(epoch, n_data, seed):
    return np.array([permute(s, epoch, n_data, seed)[0] for s in range(n_data)], dtype=np.int64)


def obs_const(likelihood, y, noise_sd):
    """What ``l`` leaves out of log p(y | eta), per observation."""
    y = np.asarray(y, dtype=np.float64)
    if likelihood == 'poisson':
        return -np.array([math.lgamma(v + 1.0) for v in y])
    if likelihood == 'gaussian':
        return np.full(y.shape, -math.log(noise_sd) - 0.5 * LOG_2PI)
    return np.zeros(y.shape)


class MinibatchOracle:
    """Batch ``idx`` of the data ``(X, y)``: the density ``f_t`` above."""

    def __init__(self, X, y, idx, likelihood='logistic', prior_sd=10.0, noise_sd=1.0):
        X, y = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64).ravel()
        self.idx = np.asarray(idx, dtype=np.int64)
        self.Xb, self.yb = X[self.idx], y[self.idx]
        self.n_data, self.dim = X.shape
        self.batch_size = self.idx.size
        self.scale = self.n_data / self.batch_size
        self.likelihood, self.prior_sd, self.noise_sd = likelihood, float(prior_sd), float(noise_sd)
        self.const_full = math.fsum(obs_const(likelihood, y, self.noise_sd))
        self.const_batch = obs_const(likelihood, self.yb, self.noise_sd)

    @staticmethod
    def _as2d(x):
        x = np.asarray(x, dtype=np.float64)
        return x[np.newaxis, :] if x.ndim == 1 else x

    def pointwise(self, theta):
        """(N, B): log p(y_j | eta_j) of the batch's observations, normalised, unscaled."""
        return terms(self.likelihood, self.yb, self._as2d(theta) @ self.Xb.T, self.noise_sd)[0]

    def log_prior(self, theta):
        theta = self._as2d(theta)
        return -0.5 * np.sum(theta * theta, axis=1) / self.prior_sd ** 2 - self.dim * (math.log(self.prior_sd) + 0.5 * LOG_2PI)

    def logp(self, theta):
        bare = self.pointwise(theta) - self.const_batch[None, :]
        return self.scale * np.sum(bare, axis=1) + self.const_full + self.log_prior(theta)

    def grad(self, theta):
        theta = self._as2d(theta)
        r = terms(self.likelihood, self.yb, theta @ self.Xb.T, self.noise_sd)[1]
        return self.scale * (r @ self.Xb) - theta / self.prior_sd ** 2
