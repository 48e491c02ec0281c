"""Host reference of ``smc`` / ``vb_smc_run`` / ``vb_smc_reweight``: adaptive tempered sequential Monte Carlo with HMC moves
as the feature's specification states it (DESIGN.md 4.28 restates it), in numpy.

TEST INFRASTRUCTURE ONLY.  Written from the specification, not from the device code.  Base ``q0 = N(loc, diag(scale^2))``,
target ``f`` from a ``value_and_grad(x) -> (f (n,), g (n, D))`` callable, path ``beta f + (1 - beta) log q0``.  As in
``_hmc_oracle``: the standard normals are GIVEN (a callable ``stream -> (n, D)``), the accept uniforms and the stage uniform
come from ``_philox_oracle`` through ``_hmc_oracle.uniforms``, and the same ``perturb`` hook (noise of ``1e-12 max|f|`` on
values, ``1e-11 max|g|`` on gradients) makes the yardstick for tolerances: ``10 |perturbed - plain| + 1e-12 max|ref|``, and
for ``betas`` another ``2^-39`` (a near-tie bisection decision may flip; both branches end within ``2^-40`` of the root).

The run reports three margins, which the CPU test vets for every case the GPU test compares exactly:
``min_accept_margin`` (smallest ``|log u - dH|``), ``min_ancestor_margin`` (smallest ``|C_j - t_i|`` over all stages) and
``min_ess_margin`` (smallest ``|E(1 - beta) - ess_target|`` at the "is this the last stage" test).
"""
import numpy as np

import _hmc_oracle as HO

HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)
BISECTIONS = 40
BETA_SLACK = 2.0 ** -39
MIN_ACCEPT_MARGIN, MIN_ANCESTOR_MARGIN, MIN_ESS_MARGIN = 1e-6, 1e-9, 1e-6


class SmcNumericError(ValueError):
    """What the device reports as VB_ERR_NUMERIC."""


def log_base_from_z(z, scale):
    return np.sum(-0.5 * z * z - np.log(scale) - HALF_LOG_2PI, axis=-1)


def log_base(x, loc, scale):
    return log_base_from_z((x - loc) / scale, scale)


def ess_fraction(v, delta):
    """``E(delta) = (sum e^{delta v})^2 / (n sum e^{2 delta v})``; a ``-inf`` entry has weight 0."""
    with np.errstate(all='ignore'):
        w = np.where(v == -np.inf, 0.0, np.exp(delta * np.where(v == -np.inf, 0.0, v)))
    return float(w.sum() ** 2 / (v.size * np.sum(w * w))), w


def systematic(w, uniform):
    """``(ancestors, margin)``: ``C`` the inclusive prefix sums of ``w`` over their total, ``t_i = (i + U) / n``,
    ``a_i = min(#{j : C_j <= t_i}, n - 1)``; ``margin`` the smallest ``|C_j - t_i|``."""
    n = w.size
    c = np.cumsum(w)
    c = c / c[-1]
    t = (np.arange(n) + uniform) / n
    idx = np.searchsorted(c, t, side='right')
    anc = np.minimum(idx, n - 1).astype(np.int64)
    near = np.minimum(np.abs(c[np.minimum(idx, n - 1)] - t), np.where(idx > 0, np.abs(c[np.maximum(idx - 1, 0)] - t), np.inf))
    return anc, float(near.min())


def reweight(u, beta_prev, ess_target, uniform):
    """One stage's reweight and resample.  Returns a dict: ``beta``, ``delta``, ``log_z_inc``, ``ess``, ``weights``,
    ``ancestors``, ``ancestor_margin``, ``ess_margin``, ``last``."""
    u = np.asarray(u, dtype=np.float64)
    n = u.size
    if np.any(np.isnan(u)) or np.any(u == np.inf):
        raise SmcNumericError('a log weight is NaN or +inf')
    if np.all(u == -np.inf):
        raise SmcNumericError('every log weight is -inf')
    umax = float(np.max(u))
    v = u - umax
    full = 1.0 - beta_prev
    e_full, _ = ess_fraction(v, full)
    last = e_full >= ess_target
    if last:
        delta, beta = full, 1.0
    else:
        lo, hi = 0.0, full
        for _ in range(BISECTIONS):
            mid = 0.5 * (lo + hi)
            if ess_fraction(v, mid)[0] >= ess_target:
                lo = mid
            else:
                hi = mid
        delta = lo
        if delta == 0.0:
            raise SmcNumericError('delta = 0 after the search')
        beta = beta_prev + delta
    e, w = ess_fraction(v, delta)
    inc = delta * umax + float(np.log(w.sum() / n))
    anc, margin = systematic(w, uniform)
    return dict(beta=beta, delta=delta, log_z_inc=inc, ess=n * e, weights=w, ancestors=anc, ancestor_margin=margin,
                ess_margin=abs(e_full - ess_target), last=last)


def run(value_and_grad, loc, scale, normals, *, n_particles, ess_target=0.5, n_moves=2, n_leapfrog=8, step_size=None,
        target_accept=0.8, adapt_rate=0.5, max_stages=200, seed=1, stream_offset=0, perturb=None):
    """The whole run.  ``normals(stream) -> (n, D)``.  Returns what ``smc`` returns (without ``mean`` / ``sd`` rounding
    concerns: they are plain numpy moments) plus ``log_base`` and the three margins."""
    vg = HO.perturbed(value_and_grad, perturb)
    loc, scale = np.asarray(loc, dtype=np.float64), np.asarray(scale, dtype=np.float64)
    n, d = int(n_particles), loc.size
    inv_mass = scale * scale
    s0 = int(stream_offset)
    step_size = d ** -0.25 if step_size is None else float(step_size)
    z = np.asarray(normals(s0), dtype=np.float64)
    x = loc + scale * z
    lq = log_base_from_z(z, scale)
    f, g = vg(x)
    f, g = np.array(f, dtype=np.float64), np.array(g, dtype=np.float64)
    beta, log_eps, eps = 0.0, float(np.log(step_size)), step_size
    betas, incs, ess, accept_hist, step_hist, n_acc, ancestors = [], [], [], [], [], [], []
    n_div = 0
    m_acc, m_anc, m_ess = np.inf, np.inf, np.inf
    k = 0
    while beta < 1.0:
        if k == max_stages:
            raise SmcNumericError('beta = %g after max_stages = %d stages' % (beta, max_stages))
        first = s0 + 1 + k * n_moves
        with np.errstate(invalid='ignore'):
            u = f - lq
        rw = reweight(u, beta, ess_target, HO.uniforms(seed, first, 1)[1])
        beta = rw['beta']
        betas.append(beta), incs.append(rw['log_z_inc']), ess.append(rw['ess']), ancestors.append(rw['ancestors'])
        m_anc, m_ess = min(m_anc, rw['ancestor_margin']), min(m_ess, rw['ess_margin'])
        a = rw['ancestors']
        x, f, g, lq = x[a], f[a], g[a], lq[a]
        omb = 1.0 - beta

        def tempered(gx, xx):
            return beta * gx - omb * ((xx - loc) / inv_mass)

        for j in range(n_moves):
            s = first + j
            uacc, _ = HO.uniforms(seed, s, n)
            p = np.asarray(normals(s), dtype=np.float64) / scale
            with np.errstate(all='ignore'):
                h0 = -(beta * f + omb * lq) + 0.5 * np.sum(inv_mass * p * p, axis=1)
                pp = p + 0.5 * eps * tempered(g, x)
                xp = x.copy()
                for l in range(n_leapfrog):
                    xp = xp + eps * inv_mass * pp
                    fp, gp = vg(xp)
                    fp, gp = np.array(fp, dtype=np.float64), np.array(gp, dtype=np.float64)
                    pp = pp + (0.5 * eps if l + 1 == n_leapfrog else eps) * tempered(gp, xp)
                lqp = log_base(xp, loc, scale)
                h1 = -(beta * fp + omb * lqp) + 0.5 * np.sum(inv_mass * pp * pp, axis=1)
                dh = h0 - h1
                div = ~np.isfinite(dh) | (h1 - h0 > HO.DIVERGENCE)
                prob = np.where(div, 0.0, np.minimum(1.0, np.exp(np.where(div, 0.0, dh))))
                log_u = np.log(uacc)
                acc = ~div & (log_u < dh)
                if np.any(~div):
                    m_acc = min(m_acc, float(np.min(np.abs(log_u - dh)[~div])))
            x = np.where(acc[:, None], xp, x)
            g = np.where(acc[:, None], gp, g)
            f = np.where(acc, fp, f)
            lq = np.where(acc, lqp, lq)
            abar = prob.sum() / n
            accept_hist.append(abar), step_hist.append(eps), n_acc.append(int(acc.sum()))
            n_div += int(div.sum())
            log_eps = log_eps + adapt_rate * (abar - target_accept)
            eps = float(np.exp(log_eps))
        k += 1
    log_ev = 0.0
    for inc in incs:
        log_ev += inc
    shape = (k, n_moves)
    return dict(particles=x, logp=f, log_base=lq, log_evidence=log_ev, betas=np.array(betas), log_z_increments=np.array(incs),
                ess=np.array(ess), accept_prob=np.array(accept_hist).reshape(shape),
                n_accepted=np.array(n_acc, dtype=np.int64).reshape(shape),
                step_size_history=np.array(step_hist).reshape(shape), step_size=eps, n_stages=k, n_divergent=n_div,
                ancestors=np.array(ancestors, dtype=np.int64), mean=x.mean(axis=0),
                sd=x.std(axis=0, ddof=1) if n > 1 else np.full(d, np.nan), next_stream=s0 + 1 + k * n_moves,
                min_accept_margin=m_acc, min_ancestor_margin=m_anc, min_ess_margin=m_ess)


def philox_normals(seed, n, d):
    """``stream -> (n, D)`` standard normals from the host Philox reference, cached per stream (fp64 roundings of the
    long-double values: within an ulp or two of the device's; for the tests that have no device)."""
    from _philox_oracle import normals
    cache = {}

    def fn(stream):
        if stream not in cache:
            cache[stream] = normals(seed, stream, 0, n, d)[0].astype(np.float64)
        return cache[stream]
    return fn


OUTPUTS = ('particles', 'logp', 'betas', 'log_z_increments', 'log_evidence', 'ess', 'accept_prob', 'step_size_history')


def tolerances(ref, pert, keys=OUTPUTS):
    out = {}
    for k in keys:
        a, b = np.asarray(ref[k], dtype=np.float64), np.asarray(pert[k], dtype=np.float64)
        out[k] = 10.0 * float(np.max(np.abs(b - a))) + 1e-12 * float(np.max(np.abs(a))) + (BETA_SLACK if k == 'betas' else 0.0)
    return out


# ---- vb_smc_reweight: the inputs the CPU test vets and the GPU test uses ------------------------------------------------------
REWEIGHT_SIZES = (1, 2, 63, 64, 65, 257, 1025, 4097)
REWEIGHT_KINDS = ('normal', 'neginf', 'heavy')
REWEIGHT_ESS = 0.5
# seeds moved off an input whose ancestor margin fell below MIN_ANCESTOR_MARGIN on the host (tests/test_smc_cpu.py vets all)
REWEIGHT_RESEED = {}


def reweight_input(kind, n):
    """``(u, beta_prev, uniform)`` of one comparison.  ``normal``: std 3; ``neginf``: the same with about a third of the
    entries ``-inf`` (never the first: at least one finite); ``heavy``: Student-t with 3 degrees of freedom scaled to a
    standard deviation of about 30."""
    seed = REWEIGHT_RESEED.get((kind, n), 1000 * REWEIGHT_KINDS.index(kind) + n)
    rng = np.random.RandomState(seed)
    if kind == 'heavy':
        u = 30.0 / np.sqrt(3.0) * rng.standard_t(3, size=n) - 50.0
    else:
        u = 3.0 * rng.randn(n) + 10.0
    if kind == 'neginf':
        drop = rng.rand(n) < 1.0 / 3.0
        drop[0] = False
        u[drop] = -np.inf
    return u, float(0.25 * rng.rand()), float(rng.rand())


# ---- run parity: cases, bases and seeds as functions of the case alone ----------------------------------------------------------
PARITY_PARTICLES = (1, 5, 64, 257)
PARITY_MAX_STAGES = 50
PARITY_ESS = 0.8               # (a high target: more, shorter stages -- at least 4 at n >= 64 even for D = 1)
PARITY_MIN_STAGES = 4
# seeds moved off a case one of whose margins fell short on the host, or whose perturbed run took another decision than the
# plain one -- a diverging trajectory's huge |f| scales the noise of the whole batch -- (tests/test_smc_cpu.py vets every case)
PARITY_RESEED = {('gauss', 64, 9): 90001, ('funnel', 64, 2): 90002, ('source', 64, 7): 90003, ('source', 257, 7): 90006}


def parity_base(kind, d, spec, rng):
    """A deliberately poor base: the target's rough centre shifted by 2 base scales per coordinate (random signs), its
    rough scale times 1.5 e^{0.2 N(0,1)}."""
    if kind == 'gauss':
        centre, ref = spec['mean'], spec['sd']
    elif kind == 'corr':
        centre, ref = spec['mean'], np.sqrt(np.diag(spec['cov']))
    else:
        centre, ref = np.zeros(d), np.ones(d)
    scale = ref * 1.5 * np.exp(0.2 * rng.randn(d))
    loc = centre + 2.0 * scale * np.where(rng.rand(d) < 0.5, -1.0, 1.0)
    return loc, scale


def parity_cases(kind, n):
    """Every (d, n_moves, n_leapfrog) of the grid for one model and particle count: dicts with ``key``, ``d``, ``n``,
    ``n_moves``, ``n_leapfrog``, ``seed``, ``loc``, ``scale``, ``step_size``, ``stream_offset``."""
    out = []
    for d in HO.parity_dims(kind):
        _, spec = HO.parity_problem(kind, d)
        for n_moves in (1, 2):
            for n_leapfrog in (1, 3):
                idx = len(out)
                key = (kind, n, idx)
                seed = PARITY_RESEED.get(key, 20000 + 1000 * HO.PARITY_MODELS.index(kind) + 100 * PARITY_PARTICLES.index(n)
                                         + idx + 1)
                loc, scale = parity_base(kind, d, spec, np.random.RandomState(seed))
                out.append(dict(key=key, d=d, n=n, n_moves=n_moves, n_leapfrog=n_leapfrog, seed=seed, loc=loc, scale=scale,
                                step_size=0.4 * d ** -0.25, stream_offset=3))
    return out


def run_case(host_model, case, normals, perturb=None, **override):
    kw = dict(n_particles=case['n'], ess_target=PARITY_ESS, n_moves=case['n_moves'], n_leapfrog=case['n_leapfrog'],
              step_size=case['step_size'], target_accept=0.8, adapt_rate=0.5, max_stages=PARITY_MAX_STAGES, seed=case['seed'],
              stream_offset=case['stream_offset'], perturb=perturb)
    kw.update(override)
    return run(HO.value_and_grad_of(host_model), case['loc'], case['scale'], normals, **kw)


# ---- statistics against closed forms ----------------------------------------------------------------------------------------------
# Three moves of three leapfrog steps: with step sizes near 0.6 and targets 1.5 times narrower than the metric, eight steps
# are close to a whole period of the Gaussian targets' orbits (no jitter), where the moves hardly mix; the oracle's
# log-evidence errors then spread over 0.8 instead of 0.03 - 0.1, and the bounds below would tell little.
STAT_PARTICLES, STAT_MOVES, STAT_LEAPFROG, STAT_ESS = 1024, 3, 3, 0.5
STAT_SEEDS = (1, 2, 3, 4, 5, 6, 7, 8)


def stat_config(name):
    """``(host model, exact mean, exact sd, exact log evidence, loc, scale, spec)``: (a) the diagonal Gaussian of
    ``_hmc_oracle.stat_config('a')`` (normalised: log Z = 0), (b) its conjugate linear regression, whose log evidence
    ``_laplace_oracle.conjugate_linear`` computes.  The bases are poor in the way of ``parity_base``."""
    host, mean, cov, _, _, spec = HO.stat_config(name)
    sd = np.sqrt(np.diag(cov))
    if name == 'a':
        log_z = 0.0
    else:
        import _laplace_oracle as LA
        log_z = LA.conjugate_linear(spec['X'], spec['y'], spec['prior_sd'], spec['noise_sd'])[3]
    rng = np.random.RandomState(50 if name == 'a' else 51)
    scale = sd * 1.5 * np.exp(0.2 * rng.randn(sd.size))
    loc = mean + 2.0 * scale * np.where(rng.rand(sd.size) < 0.5, -1.0, 1.0)
    return host, mean, sd, log_z, loc, scale, spec


def stat_figures(res, mean, sd, log_z):
    """``(log evidence error, mean error / sd, sd ratio error)``."""
    return (float(res['log_evidence'] - log_z), float(np.max(np.abs(res['mean'] - mean) / sd)),
            float(np.max(np.abs(res['sd'] / sd - 1.0))))


def stat_run(name, seed, perturb=None):
    host, mean, sd, log_z, loc, scale, _ = stat_config(name)
    res = run(HO.value_and_grad_of(host), loc, scale, philox_normals(seed, STAT_PARTICLES, loc.size),
              n_particles=STAT_PARTICLES, ess_target=STAT_ESS, n_moves=STAT_MOVES, n_leapfrog=STAT_LEAPFROG, seed=seed,
              perturb=perturb)
    return res, stat_figures(res, mean, sd, log_z)


# The oracle's own figures over STAT_SEEDS (python tests/_smc_oracle.py prints them), from which the bounds follow: four times
# the sample standard deviation (ddof = 1) of the log-evidence errors, four times the worst mean error and sd ratio error.
STAT_ORACLE = {
    'a': [
        (0.0339056665097508, 0.05761304746427031, 0.07502573892477193),      # seed 1: 12 stages
        (-0.02822708311913935, 0.058837733483801856, 0.04717217498852899),   # seed 2
        (0.043807463855725315, 0.06339498084651479, 0.08996954208959274),    # seed 3
        (0.019786839020878078, 0.06437824237023557, 0.06366238859707696),    # seed 4
        (-0.031248410989999975, 0.06962234527584307, 0.05665466836469868),   # seed 5
        (-0.2967469052817778, 0.0751434804503554, 0.033814476611528255),     # seed 6
        (-0.2422474046594727, 0.047494565285932794, 0.05385795249774916),    # seed 7
        (0.09032627997556508, 0.10612878298034518, 0.053236139028107754),    # seed 8
    ],
    'b': [
        (0.2794703757149932, 0.042414248646874056, 0.09363772464602416),     # seed 1: 8 stages
        (0.07150053896793906, 0.056833833481933126, 0.06246997228868667),    # seed 2
        (0.0213590460413684, 0.054825225332528954, 0.03207630023673769),     # seed 3
        (0.06977045016697048, 0.07347410158740207, 0.057511033684673474),    # seed 4
        (-0.06895363246945863, 0.07169918353286106, 0.04424930365828472),    # seed 5
        (-0.07655909817304973, 0.05776088912805983, 0.07466443030907133),    # seed 6
        (-0.05419347228882998, 0.06945778309378119, 0.033297816082863085),   # seed 7
        (0.03287904373655692, 0.02689766256153931, 0.06611904099006394),     # seed 8
    ],
}
# the resulting constants (stat_bounds): 'a' 0.564 / 0.425 / 0.360, 'b' 0.463 / 0.294 / 0.375
STAT_TEST_SEED = {'a': 1, 'b': 2}        # a seed at which the oracle itself meets the bounds (tests/test_smc_cpu.py asserts it)


def stat_bounds(name):
    rows = np.array(STAT_ORACLE[name])
    return 4.0 * float(np.std(rows[:, 0], ddof=1)), 4.0 * float(np.max(rows[:, 1])), 4.0 * float(np.max(rows[:, 2]))


if __name__ == '__main__':
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    for cfg in ('a', 'b'):
        print("    '%s': [" % cfg)
        for sd_ in STAT_SEEDS:
            r, fig = stat_run(cfg, sd_)
            print('        (%r, %r, %r),      # seed %d: %d stages' % (fig + (sd_, r['n_stages'])))
        print('    ],')
