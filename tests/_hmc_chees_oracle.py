"""Host reference of ``hmc(..., trajectory='chees')`` / ``vb_hmc_run_chees``: ChEES-HMC (Hoffman, Radul & Sountsov 2021) as the
feature's specification states it (DESIGN.md 4.25 restates it), in numpy, for the diagonal and the dense metric.

TEST INFRASTRUCTURE ONLY.  Written from the specification, not from the device code.  One trajectory length ``T`` is shared by
the chains.  Iteration ``t`` (Philox stream ``s = stream_offset + t``) runs ``L_t = clamp(ceil(tau_t / eps_t), 1,
max_leapfrog)`` leapfrog steps, ``tau_t = h_s T_t``, ``h_s = (bitreverse32(low32(s + 1)) + 0.5) 2^-32``.  A warm-up
iteration forms, from the states ``x``, the proposals ``x'``, the velocities ``v'`` at the proposals and the acceptance
probabilities ``a``, over the usable chains (finite log density at the proposal)

    crit_c = (|x'_c - mean x'|^2 - |x_c - mean x|^2) ((x'_c - mean x') . v'_c),     g = tau_t sum a_c crit_c / sum a_c

(``mean x`` over all chains, ``mean x'`` over the usable ones) and takes an Adam step without first moment on ``log T``
(``beta_2 = 0.95``, learning rate 0.025), clamps ``log T`` to ``[log eps_base, log(max_leapfrog eps_base)]`` and averages
it with the weights ``m^-0.75``; sampling uses the exponential of the average.  Momenta, energies, the divergence rule, the
accept test, dual averaging, the jitter, Welford and the window moments are ``_hmc_oracle``'s and ``_hmc_metric_oracle``'s,
whose pieces (``uniforms``, ``perturbed``, ``trajectory``, ``energy``, the case models, the window schedule and metric) are
imported; the dense leapfrog is inline in ``_hmc_metric_oracle.run`` and is restated here line by line, since the criterion
needs the proposal and the final momenta, which that function does not return.
"""
import numpy as np

import _hmc_metric_oracle as MO
import _hmc_oracle as HO
from _hmc_oracle import DIVERGENCE, GAMMA, KAPPA, T0, perturbed, uniforms

BETA2, ADAM_EPS, LR = 0.95, 1e-8, 0.025


def perturbed_in_groups(value_and_grad, rng, groups):
    """``_hmc_oracle.perturbed`` applied to each group of rows on its own: the hook's noise is ``1e-12 max|f|`` and
    ``1e-11 max|g|`` over the rows it sees, which says nothing about a batch in which a few rows are 1e260 by design."""
    if rng is None:
        return value_and_grad

    def fn(x):
        f, g = value_and_grad(x)
        f, g = np.array(f, dtype=np.float64), np.array(g, dtype=np.float64)
        for rows in groups:
            f[rows], g[rows] = perturbed(lambda _: (f[rows], g[rows]), rng)(None)
        return f, g
    return fn


def halton(s):
    """``h_s``: the base-2 radical inverse of ``low32(s + 1)``, moved half a cell into (0, 1); exact in fp64."""
    n = (int(s) + 1) & 0xFFFFFFFF
    return (int('{:032b}'.format(n)[::-1], 2) + 0.5) * 2.0 ** -32


def n_steps(tau, eps, max_leapfrog):
    """``(L, margin)``: ``clamp(ceil(tau / eps), 1, max_leapfrog)`` and the distance of ``tau / eps`` from an integer where
    the clamp is not active (``inf`` where it is)."""
    ratio = tau / eps
    if not np.isfinite(ratio):
        return (max_leapfrog if ratio > 0 else 1), np.inf
    steps = int(min(max(np.ceil(ratio), 1.0), float(max_leapfrog)))
    active = ratio > max_leapfrog or ratio <= 0.0
    return steps, (np.inf if active else abs(ratio - np.round(ratio)))


def initial_state(trajectory_length):
    return np.array([np.log(trajectory_length), 0.0, np.log(trajectory_length), 0.0])


def run(value_and_grad, x0, normals, *, L=None, inv_mass=None, n_warmup=0, n_draws=1, max_leapfrog=1, step_size=1.0,
        traj_state=None, trajectory_length=None, trajectory_lr=LR, target_accept=0.8, jitter=0.0, seed=1, stream_offset=0,
        thin=1, perturb=None, perturb_groups=None, moment_shift=None, t0=0):
    """One engine call.  ``L`` (D x D, lower) selects the dense metric, ``inv_mass`` (D,) the diagonal one; ``traj_state`` is
    ``(log T, v, log T_bar, m)`` (default: ``initial_state(trajectory_length)``, ``trajectory_length`` defaulting to
    ``step_size``).  Returns what ``_hmc_metric_oracle.run`` returns plus ``traj_state`` (after the call),
    ``trajectory_history``, ``n_leapfrog_history``, ``trajectory_length`` (``exp(log T_bar)`` after the call), ``usable``
    (T x C), ``a`` (T x C), ``adapted`` (T; whether the iteration changed ``(log T, v)`` by the Adam step) and
    ``min_step_margin``.  ``perturb_groups`` (lists of rows) makes the perturbation hook act on each group separately."""
    assert (L is None) != (inv_mass is None)
    dense = L is not None
    vg = perturbed(value_and_grad, perturb) if perturb_groups is None else perturbed_in_groups(value_and_grad, perturb,
                                                                                               perturb_groups)
    x = np.array(x0, dtype=np.float64)
    n_chains, d = x.shape
    if dense:
        L = np.tril(np.asarray(L, dtype=np.float64))
    else:
        inv_mass = np.asarray(inv_mass, dtype=np.float64)
    if traj_state is None:
        traj_state = initial_state(step_size if trajectory_length is None else trajectory_length)
    log_t, v2, log_t_bar, m_traj = (float(e) for e in traj_state)
    n_iter = n_warmup + n_draws
    f, g = vg(x)
    f, g = np.array(f, dtype=np.float64), np.array(g, dtype=np.float64)
    mu = np.log(10.0 * step_size)
    hbar, log_eps_bar, base = 0.0, 0.0, float(step_size)
    step_hist, accept_hist, traj_hist = np.empty(n_iter), np.empty(n_iter), np.empty(n_iter)
    leap_hist = np.zeros(n_iter, dtype=np.int64)
    accepted, divergent = np.zeros((n_iter, n_chains), dtype=bool), np.zeros((n_iter, n_chains), dtype=bool)
    usable_all, a_all, adapted = np.ones((n_iter, n_chains), dtype=bool), np.empty((n_iter, n_chains)), np.zeros(n_iter, bool)
    draws, logp = [], []
    mean, m2, count, n_div = np.zeros((n_chains, d)), np.zeros((n_chains, d)), np.zeros(n_chains), 0
    s1 = s2 = None
    if moment_shift is not None:
        moment_shift = np.asarray(moment_shift, dtype=np.float64)
        s1, s2 = np.zeros(d), np.zeros((d, d) if dense else d)
    min_margin, min_step_margin = np.inf, np.inf
    for t in range(n_iter):
        s = stream_offset + t
        u, v = uniforms(seed, s, n_chains)
        eps = base * (1.0 + jitter * (2.0 * v - 1.0))
        step_hist[t] = eps
        traj = float(np.exp(log_t if t < n_warmup else log_t_bar))
        tau = halton(s) * traj
        n_leapfrog, step_margin = n_steps(tau, eps, max_leapfrog)
        traj_hist[t], leap_hist[t] = traj, n_leapfrog
        min_step_margin = min(min_step_margin, step_margin)
        z = np.asarray(normals(t0 + t) if callable(normals) else normals[t0 + t], dtype=np.float64)
        with np.errstate(all='ignore'):
            if dense:
                r = z.copy()
                h0 = -f + 0.5 * np.sum(r * r, axis=1)
                r = r + 0.5 * eps * (g @ L)
                xp, fp, gp = x, f, g
                for l in range(n_leapfrog):
                    xp = xp + eps * (r @ L.T)
                    fp, gp = vg(xp)
                    r = r + (0.5 * eps if l + 1 == n_leapfrog else eps) * (gp @ L)
                h1 = -fp + 0.5 * np.sum(r * r, axis=1)
                vel = r @ L.T
            else:
                p = z / np.sqrt(inv_mass)
                h0 = HO.energy(f, p, inv_mass)
                xp, pp, fp, gp = HO.trajectory(vg, x, p, g, eps, n_leapfrog, inv_mass)
                h1 = HO.energy(fp, pp, inv_mass)
                vel = inv_mass * pp                    # (pp has the last half kick)
            crit, usable = None, np.isfinite(fp)
            if t < n_warmup:                           # before the accept step overwrites anything
                dx = x - x.mean(axis=0)
                dxp = xp - (xp[usable].mean(axis=0) if np.any(usable) else 0.0)
                crit = (np.sum(dxp * dxp, axis=1) - np.sum(dx * dx, axis=1)) * np.sum(dxp * vel, axis=1)
            dh = h0 - h1
            div = ~np.isfinite(dh) | (h1 - h0 > DIVERGENCE)
            a = np.where(div, 0.0, np.minimum(1.0, np.exp(np.where(div, 0.0, dh))))
            log_u = np.log(u)
            acc = ~div & (log_u < dh)
            if np.any(~div):
                min_margin = min(min_margin, float(np.min(np.abs(log_u - dh)[~div])))
        x = np.where(acc[:, None], xp, x)
        g = np.where(acc[:, None], gp, g)
        f = np.where(acc, fp, f)
        accepted[t], divergent[t], usable_all[t], a_all[t] = acc, div, usable, a
        abar = a.sum() / n_chains
        accept_hist[t] = abar
        if s1 is not None:
            xc = x - moment_shift
            s1 = s1 + xc.sum(axis=0)
            s2 = s2 + (xc.T @ xc if dense else np.sum(xc * xc, axis=0))
        if t < n_warmup:
            m = t + 1.0
            hbar = (1.0 - 1.0 / (m + T0)) * hbar + (target_accept - abar) / (m + T0)
            log_eps = mu - np.sqrt(m) / GAMMA * hbar
            eta = m ** -KAPPA
            log_eps_bar = eta * log_eps + (1.0 - eta) * log_eps_bar
            base = float(np.exp(log_eps) if t + 1 < n_warmup else np.exp(log_eps_bar))
            # the trajectory length
            with np.errstate(all='ignore'):
                sum_a = float(np.sum(a[usable]))
                ghat = float(tau * np.sum(a[usable] * crit[usable]) / sum_a) if sum_a != 0.0 else np.nan
            m_traj += 1.0
            if sum_a != 0.0 and np.isfinite(ghat):
                v2 = BETA2 * v2 + (1.0 - BETA2) * ghat * ghat
                log_t = log_t + trajectory_lr * ghat / (np.sqrt(v2 / (1.0 - BETA2 ** m_traj)) + ADAM_EPS)
                adapted[t] = True
            log_t = float(min(max(log_t, np.log(base)), np.log(max_leapfrog * base)))
            eta = m_traj ** -KAPPA
            log_t_bar = eta * log_t + (1.0 - eta) * log_t_bar
        else:
            k = t - n_warmup + 1.0
            delta = x - mean
            mean = mean + delta / k
            m2 = m2 + delta * (x - mean)
            count += acc
            n_div += int(div.sum())
            if (t - n_warmup) % thin == 0:
                draws.append(x.copy())
                logp.append(f.copy())
    chain_var = None
    if n_draws > 0:
        with np.errstate(all='ignore'):
            chain_var = m2 / (n_draws - 1.0) if n_draws > 1 else np.full_like(m2, np.nan)
    return dict(draws=np.array(draws).reshape(-1, n_chains, d), logp=np.array(logp).reshape(-1, n_chains), last=x,
                chain_mean=mean, chain_var=chain_var, accept_rate=count / max(n_draws, 1), accept_prob=accept_hist,
                step_size_history=step_hist, step_size=base, n_divergent=n_div, accepted=accepted, divergent=divergent,
                min_margin=min_margin, next_stream=stream_offset + n_iter, moment_sum=s1, moment_m2=s2,
                traj_state=np.array([log_t, v2, log_t_bar, m_traj]), trajectory_history=traj_hist,
                n_leapfrog_history=leap_hist, trajectory_length=np.float64(np.exp(log_t_bar)), usable=usable_all, a=a_all,
                adapted=adapted, min_step_margin=min_step_margin)


def run_adaptive(value_and_grad, x0, normals, *, dense, inv_mass, n_warmup, n_draws, max_leapfrog, step_size=1.0,
                 trajectory_length=None, trajectory_lr=LR, target_accept=0.8, jitter=0.0, seed=1, stream_offset=0, thin=1,
                 perturb=None):
    """``_hmc_metric_oracle.run_adaptive`` with ``run`` above as the engine call: the segments continue the trajectory state
    as they continue the states, the step and the stream."""
    wins = MO.windows(n_warmup)
    segments = ([(wins[0][0], 0, False)] if wins[0][0] > 0 else []) + [(e - s, 0, True) for s, e in wins]
    segments.append((n_warmup - wins[-1][1], n_draws, False))
    metric = np.asarray(inv_mass, dtype=np.float64)
    x, step, done = np.array(x0, dtype=np.float64), float(step_size), 0
    state = initial_state(step_size if trajectory_length is None else trajectory_length)
    hist, margin, step_margin, accepted = [], np.inf, np.inf, []
    n_chains = x.shape[0]
    for seg_warmup, seg_draws, is_window in segments:
        kw = dict(L=np.linalg.cholesky(metric)) if dense else dict(inv_mass=metric)
        shift = x.mean(axis=0) if is_window else None
        res = run(value_and_grad, x, normals, n_warmup=seg_warmup, n_draws=seg_draws, max_leapfrog=max_leapfrog,
                  step_size=step, traj_state=state, trajectory_lr=trajectory_lr, target_accept=target_accept, jitter=jitter,
                  seed=seed, stream_offset=stream_offset + done, thin=thin, perturb=perturb, moment_shift=shift, t0=done, **kw)
        if is_window:
            metric = MO.window_metric(shift, res['moment_sum'], res['moment_m2'], float(n_chains * seg_warmup), dense)
        hist.append([res[k] for k in ('step_size_history', 'accept_prob', 'trajectory_history', 'n_leapfrog_history')])
        accepted.append(res['accepted'])
        margin, step_margin = min(margin, res['min_margin']), min(step_margin, res['min_step_margin'])
        x, step, state, done = res['last'], res['step_size'], res['traj_state'], done + seg_warmup + seg_draws
    for i, k in enumerate(('step_size_history', 'accept_prob', 'trajectory_history', 'n_leapfrog_history')):
        res[k] = np.concatenate([h[i] for h in hist])
    res['accepted'] = np.concatenate(accepted)
    res['trajectory_length'] = res['trajectory_history'][n_warmup]
    res.update(inv_mass=metric, adapt_windows=wins, min_margin=margin, min_step_margin=step_margin)
    return res


# ---- the cases the CPU and the GPU tests share --------------------------------------------------------------------------------
OUTPUTS = ('draws', 'logp', 'last', 'chain_mean', 'chain_var', 'accept_prob', 'step_size_history', 'trajectory_history',
           'trajectory_length')
PARITY_MODELS = ('gauss', 'funnel', 'logistic', 'source')
PARITY_CHAINS = (2, 5, 64, 257)          # four chains per workgroup, the four-wave deal, the 256-thread stride
PARITY_DIMS = (1, 2, 17, 65)             # the 16-column pad, the 64-lane stride, the 64-column block
PARITY_WARMUP, PARITY_DRAWS, PARITY_MAX_LEAPFROG, PARITY_STEP, PARITY_LENGTH_STEPS = 6, 4, 5, 0.05, 30.0
MIN_STEP_MARGIN, MAX_HISTORY_SPREAD = 1e-6, 1e-6
# seeds moved off a case that misses a condition of tests/test_hmc_chees_cpu.py::test_parity_seeds (which vets every case)
RESEED = {('funnel', 257, 10): 1710311,       # the perturbation hook moved the trajectory history by 1.5e-5
          ('logistic', 257, 6): 1720307}      # an accept test decided within 5.1e-7


def parity_dims(kind):
    return PARITY_DIMS[1:] if kind == 'funnel' else PARITY_DIMS


def parity_cases(kind, n_chains):
    """Every (d, metric, jitter) of the grid for one model and chain count.  The initial trajectory length is thirty steps:
    the clamp at five steps is active at first, and once dual averaging has raised the step size ``h_s T / eps`` spreads
    over (0, 5) and the step counts over 1 .. 5.  The starting step is small because dual averaging aims at ten times the
    step it starts from, and trajectories beyond the leapfrog's stability limit amplify a rounding difference exponentially
    (``_hmc_metric_oracle.adapt_case``)."""
    out = []
    for d in parity_dims(kind):
        for dense in (False, True):
            for jitter in (0.0, 0.2):
                key = (kind, n_chains, len(out))
                seed = RESEED.get(key, 700000 + 10000 * PARITY_MODELS.index(kind) + 100 * PARITY_CHAINS.index(n_chains)
                                  + len(out) + 1)
                rng = np.random.RandomState(seed)
                x0 = (0.5 if kind == 'funnel' else 1.0) * rng.randn(n_chains, d)
                inv_mass = np.exp(0.2 * rng.randn(d))
                a = rng.randn(d, d)
                step = PARITY_STEP * d ** -0.25
                out.append(dict(key=key, d=d, dense=dense, jitter=jitter, seed=seed, x0=x0, inv_mass=inv_mass,
                                sigma=a @ a.T / d + np.eye(d), step_size=step, trajectory_length=PARITY_LENGTH_STEPS * step, thin=1,
                                stream_offset=3))
    return out


def run_case(host_model, case, normals, perturb=None, **override):
    kw = dict(n_warmup=PARITY_WARMUP, n_draws=PARITY_DRAWS, max_leapfrog=PARITY_MAX_LEAPFROG, step_size=case['step_size'],
              trajectory_length=case['trajectory_length'], target_accept=0.8, jitter=case['jitter'], seed=case['seed'],
              stream_offset=case['stream_offset'], thin=case['thin'], perturb=perturb)
    kw.update(dict(L=np.linalg.cholesky(case['sigma'])) if case['dense'] else dict(inv_mass=case['inv_mass']))
    kw.update(override)
    return run(HO.value_and_grad_of(host_model), case['x0'], normals, **kw)


def history_spread(ref, pert):
    """Largest relative difference of the perturbed oracle's trajectory history from the unperturbed one."""
    return float(np.max(np.abs(pert['trajectory_history'] / ref['trajectory_history'] - 1.0)))


# unusable chains: a funnel (the log scale v is the last coordinate) on which most chains start as the parity grid's do, two
# start at v = -300 and two at v = -4, all four with the other coordinates at +-1.  At v = -300 the gradient is of the
# order e^600: the first kick throws v beyond 1e150, v^2 overflows and the proposal's log density is not finite, whatever
# the step.  At v = -4 the first kick gains a kinetic energy of several thousand: a divergence with a finite log density.
# Neither kind of chain is ever accepted, so both occur in every iteration; the other chains do not feel them except
# through the two means.
UNUSABLE_CHAINS, UNUSABLE_DIM, UNUSABLE_SEED = 64, 3, 31
UNUSABLE_OVERFLOW, UNUSABLE_DIVERGENT = (5, 40), (17, 63)


def unusable_case(dense):
    rng = np.random.RandomState(UNUSABLE_SEED)
    x0 = 0.5 * rng.randn(UNUSABLE_CHAINS, UNUSABLE_DIM)
    a = rng.randn(UNUSABLE_DIM, UNUSABLE_DIM)
    for rows, v in ((UNUSABLE_OVERFLOW, -300.0), (UNUSABLE_DIVERGENT, -4.0)):
        x0[list(rows)] = np.array([[1.0, -1.0, v], [-1.0, 1.0, v]])
    step = PARITY_STEP * UNUSABLE_DIM ** -0.25
    wild = UNUSABLE_OVERFLOW + UNUSABLE_DIVERGENT
    groups = [[c for c in range(UNUSABLE_CHAINS) if c not in wild], list(UNUSABLE_OVERFLOW), list(UNUSABLE_DIVERGENT)]
    return dict(key=('unusable', dense), groups=groups, d=UNUSABLE_DIM, dense=dense, jitter=0.2, seed=UNUSABLE_SEED, x0=x0,
                inv_mass=np.ones(UNUSABLE_DIM), sigma=0.1 * a @ a.T / UNUSABLE_DIM + np.eye(UNUSABLE_DIM), step_size=step,
                trajectory_length=PARITY_LENGTH_STEPS * step, thin=1, stream_offset=0)


# all chains divergent in every iteration: a narrow Gaussian under a step of 10; T = 25 stays inside the clamp's interval
# while the dual averaging moves the base step (23.4 after the first iteration, 5.9 after the second and last)
REJECT_DIM, REJECT_CHAINS, REJECT_WARMUP, REJECT_STEP, REJECT_LENGTH = 3, 9, 2, 10.0, 25.0

# adaptive parity: _hmc_metric_oracle.adapt_case's problems (one window, [6, 36)), at most five steps, from T = 3 steps
ADAPT_MAX_LEAPFROG, ADAPT_LENGTH_STEPS = 5, 3.0

# statistics: _hmc_oracle.stat_config's two targets, from T = step_size (one leapfrog step)
STAT_MAX_LEAPFROG = 64
