"""Target models.

Mirrors ``viabel/models.py`` (``Model`` ``:11-77``).  The reference model is an arbitrary
Python callable differentiated by autograd; a GPU engine needs targets whose log density
and derivatives exist as device code, so the hot path accepts
:class:`DeviceModel` instances.  Calling a device model evaluates ``f(x_n)`` on the GPU
through the C ABI (``vb_model_logp``) -- same contract as ``Model.__call__``
(``models.py:27-39``): ``(N, D) -> (N,)``, and ``(D,)`` is promoted to one row
(``viabel/tests/test_models.py:14-15``).
"""
import numpy as np

from . import _lib

__all__ = ['Model', 'DeviceModel', 'GaussianModel', 'FunnelModel', 'CorrelatedGaussianModel',
           'LogisticRegressionModel', 'PoissonRegressionModel', 'LinearRegressionModel', 'SoftmaxRegressionModel',
           'MultilevelRegressionModel', 'LocationScaleRegressionModel', 'SparseRegressionModel',
           'NeuralNetRegressionModel', 'MinibatchRegressionModel', 'SourceModel', 'CallableModel']


class Model(object):
    """Base class for representing a model (``viabel/models.py:11-77``).

    A plain ``Model(log_density)`` wraps a host callable.  The objectives bind it as a
    :class:`CallableModel` (the callable is evaluated on the host between the device's sampling and
    reduction kernels, its gradient by central differences); the built-in device models and
    :class:`SourceModel` are the fast routes.
    """

    def __init__(self, log_density):
        self._log_density = log_density

    def __call__(self, model_param):
        return self._log_density(model_param)

    def constrain(self, model_param):
        raise NotImplementedError()

    @property
    def supports_tempering(self):
        return False

    def set_inverse_temperature(self, inverse_temp):
        raise NotImplementedError()


def ksd_results(ksd2, rowsums, log_weights, c, beta):
    """The dict ``ksd_from_draws`` and ``viabel_amd.ksd`` return, from what ``Engine.ksd`` gives."""
    n = rowsums.shape[0]
    if log_weights is None:
        ess = float(n)
    else:
        w = np.exp(log_weights - np.max(log_weights))
        ess = float(np.sum(w) ** 2 / np.sum(w * w))
    ksd2 = float(ksd2)
    return dict(ksd=float(np.sqrt(max(ksd2, 0.0))), ksd2=ksd2, rowsums=rowsums, ess=ess, n_samples=int(n), c=float(c),
                beta=float(beta))


class DeviceModel(Model):
    """A target whose log density / gradient / Hessian products are HIP device code."""

    def __init__(self, dim):
        self._dim = int(dim)
        super().__init__(self._device_log_density)

    @property
    def dim(self):
        return self._dim

    def device_spec(self):
        """``(model_id, dim, dparams, iparams)`` for ``vb_set_model`` (built once, then cached)."""
        spec = getattr(self, '_spec_cache', None)
        if spec is None:
            spec = self._spec_cache = self._build_spec()
        return spec

    def _build_spec(self):
        raise NotImplementedError()

    def _device_log_density(self, x):
        x = np.asarray(x, dtype=np.float64)
        one = x.ndim == 1
        if one:
            x = x[np.newaxis, :]
        if x.ndim != 2 or x.shape[1] != self._dim:
            raise ValueError('model_param must have shape (N, {0}) or ({0},)'.format(self._dim))
        eng = _lib.default_engine()
        eng.set_model(self.device_spec())
        return eng.model_logp(x)

    def _rows(self, x):
        x = np.asarray(x, dtype=np.float64)
        one = x.ndim == 1
        if one:
            x = x[np.newaxis, :]
        if x.ndim != 2 or x.shape[1] != self._dim:
            raise ValueError('model_param must have shape (N, {0}) or ({0},)'.format(self._dim))
        return np.ascontiguousarray(x), one

    _pointwise_entry = None      # the Engine method behind pointwise_log_likelihood (the classes that have one)

    def _pointwise(self, x):
        x, _ = self._rows(x)
        eng = _lib.default_engine()
        eng.set_model(self.device_spec())
        return self._pointwise_order(getattr(eng, self._pointwise_entry)(x, self.n_data))

    def _pointwise_order(self, out):
        """Hook: the engine's ``(S, n_data)`` terms in the order in which the caller gave the observations."""
        return out

    def grad(self, x):
        """Gradient of the log density at each row of ``x`` -- what ``autograd.elementwise_grad(model)`` gives in the
        reference (``objectives.py:191``; ``tests/test_models.py:13-15`` checks it) -- from the device code the
        objectives use (``vb_model_grad``).  ``x``: (N, D) or (D,); returns the same shape."""
        x, one = self._rows(x)
        eng = _lib.default_engine()
        eng.set_model(self.device_spec())
        g = eng.model_grad(x)[1]
        return g[0] if one else g

    def ksd_from_draws(self, x, log_weights=None, scale=None, c=1.0, beta=-0.5):
        """Kernel Stein discrepancy of the weighted draws ``x`` (S x D) against this model (Gorham & Mackey 2017; inverse
        multiquadric kernel ``(c^2 + |x - y|^2)^beta``): how far the draws are from the target, from the target's scores
        alone -- no normalising constant, no reference sample.  The scores are this model's device gradient at the
        draws and stay on the device (``vb_ksd``, ``Engine.ksd``).  ``log_weights`` (S,; None: uniform; normalised by the
        entry), ``scale`` (D,; None: ones): the discrepancy is that of ``x / scale``.  Returns a dict: ``ksd``
        (``sqrt(max(ksd2, 0))``), ``ksd2``, ``rowsums`` (S,; ``ksd2 = sum_i w_i rowsums[i]``), ``ess``
        (``1 / sum w^2``), ``n_samples``, ``c``, ``beta``."""
        self._refuse_ksd()
        x, _, log_weights, scale, c, beta = _lib.ksd_arguments(x, None, log_weights, scale, c, beta)
        if x.shape[1] != self._dim:
            raise ValueError('x must have shape (S, {})'.format(self._dim))
        eng = _lib.default_engine()
        eng.set_model(self.device_spec())
        ksd2, rowsums = eng.ksd(x, None, log_weights, scale, c, beta)
        return ksd_results(ksd2, rowsums, log_weights, c, beta)

    def _refuse_ksd(self):
        """Hook: ``NotImplementedError`` from the models whose scores the device cannot supply."""

    def svgd_direction(self, x, scale=None, bandwidth='median'):
        """One Stein variational gradient descent direction (Liu & Wang 2016) of the particles ``x`` (n x D) towards this
        model: ``phi(x_i) = 1/n sum_j [k(x_j, x_i) grad log p(x_j) + grad_{x_j} k(x_j, x_i)]`` with the RBF kernel
        ``exp(-|y - y'|^2 / h)`` of ``y = (x - mean) / scale``.  The scores are this model's device gradient and stay on
        the device (``vb_svgd_direction``, ``Engine.svgd_direction``).  ``scale`` (D,; None: ones); ``bandwidth``:
        ``'median'`` (``h`` = the lower median of the squared pair distances over ``log(n + 1)``) or a positive number.
        Returns a dict: ``phi`` (n x D), ``bandwidth`` (the ``h`` used) and ``logp`` (n,)."""
        self._refuse_svgd('svgd_direction()')
        x, _, scale, bandwidth = _lib.svgd_arguments(x, None, scale, bandwidth)
        if x.shape[1] != self._dim:
            raise ValueError('x must have shape (n, {})'.format(self._dim))
        eng = _lib.default_engine()
        eng.set_model(self.device_spec())
        phi, h, logp = eng.svgd_direction(x, None, scale, 'median' if bandwidth == 0.0 else bandwidth)
        return dict(phi=phi, bandwidth=h, logp=logp)

    def _refuse_svgd(self, what):
        """Hook: ``NotImplementedError`` from the models whose scores the device cannot supply."""

    def check_gradient(self, x, step=1e-6):
        """Largest deviation of the device gradient from central differences of the device log density at the rows of
        ``x``, relative to the largest gradient entry there: the check the reference runs on its models with
        ``autograd.test_util.check_vjp`` (``tests/test_models.py:13-15``).  For a ``SourceModel`` the gradient is
        hand-written code and nothing else verifies it: a value above ~1e-6 means ``grad`` does not match ``f``."""
        x, _ = self._rows(x)
        n, d = x.shape
        h = step * np.maximum(1.0, np.abs(x))                          # (N, D) per-coordinate steps
        pts = np.repeat(x[:, np.newaxis, :], 2 * d, axis=1)          # (N, 2D, D): x + h e_j, then x - h e_j
        idx = np.arange(d)
        pts[:, idx, idx] += h
        pts[:, d + idx, idx] -= h
        f = self(pts.reshape(n * 2 * d, d)).reshape(n, 2 * d)
        fd = (f[:, :d] - f[:, d:]) / (2.0 * h)
        g = self.grad(x)
        return float(np.max(np.abs(g - fd)) / max(np.max(np.abs(g)), np.max(np.abs(fd)), 1e-300))

    HESSIAN_DIFFERENCE_MAX_DIM = 4096      # the difference route evaluates 4 D + 1 gradients of D entries in one call

    def hessian(self, x):
        """Hessian of the log density at each row of ``x``: (D,) -> (D, D), (N, D) -> (N, D, D).  This default serves
        every device model: fourth-order central differences of the device gradient with step
        ``h = 2e-3 max(1, max|x|)`` -- the stencil of the source models' control variates -- all ``4 D + 1`` points in
        one ``grad`` call, the result symmetrised; relative error ~1e-11 for smooth densities.  ``dim`` above
        ``HESSIAN_DIFFERENCE_MAX_DIM`` raises ``NotImplementedError``.  The flat regression targets and the two Gaussian
        targets override it with exact Hessians."""
        d = self._dim
        if d > self.HESSIAN_DIFFERENCE_MAX_DIM:
            raise NotImplementedError(
                'the difference route of hessian() takes at most {} dimensions (4 D + 1 gradient evaluations of D entries '
                'each); {} has {}'.format(self.HESSIAN_DIFFERENCE_MAX_DIM, type(self).__name__, d))
        x, one = self._rows(x)
        out = np.empty((x.shape[0], d, d))
        eye = np.eye(d)
        for n, xn in enumerate(x):
            h = 2e-3 * max(1.0, float(np.max(np.abs(xn))))
            pts = np.concatenate([xn[None, :], xn + h * eye, xn - h * eye, xn + 2 * h * eye, xn - 2 * h * eye])
            g = self.grad(pts)
            d1 = g[1:1 + d] - g[1 + d:1 + 2 * d]
            d2 = g[1 + 2 * d:1 + 3 * d] - g[1 + 3 * d:]
            ht = (8.0 * d1 - d2) / (12.0 * h)              # row j = d grad f / d x_j
            out[n] = 0.5 * (ht + ht.T)
        return out[0] if one else out

    def _value_grad_hessian(self, x, want_hessian=True):
        """``(f, grad, hessian or None)`` at the single point ``x`` (D,): the one hook :meth:`find_mode` and
        ``laplace_approximation`` evaluate the model through."""
        x = np.asarray(x, dtype=np.float64)
        return float(self(x)[0]), self.grad(x), self.hessian(x) if want_hessian else None

    def find_mode(self, x0=None, max_iter=100, tol=1e-10):
        """Mode of the log density by damped Newton ascent from ``x0`` (None: zeros).  Per iteration: ``(f, g, H)`` from
        :meth:`_value_grad_hessian`; ``(-H) delta = g`` by Cholesky, with a ridge ``lambda I`` -- from
        ``1e-6 max|diag H|``, times 10 until the factorisation succeeds with every squared pivot at least ``lambda / 1000``
        -- where ``-H`` is not positive definite;
        backtracking ``t = 1, 1/2, ...`` (at most 30 halvings, value-only evaluations) while
        ``f(x + t delta) < f(x) + 1e-4 t g' delta``.  Close to the mode the values cannot order the two points any more
        (the gain ``g' delta / 2`` a Newton step promises falls below ``64 eps max(1, |f|)``, the rounding of ``f``
        itself): a full step that fails the test there is taken all the same -- it is accurate where the comparison is
        not.  A step with ``max|t delta| <= tol max(1, max|x|)`` is still applied, ``(f, g, H)`` are evaluated at the
        result and the search stops.  Returns a dict: ``mode``, ``value``, ``grad``, ``hessian``, ``n_iter`` (steps above
        that threshold: the closing one is not counted, so a quadratic takes one), ``converged``.  Running out of
        iterations or halvings gives ``converged=False`` and a warning, not an exception."""
        from ._newton import newton_ascent      # (the host LAPACK calls live there: this module stays free of scipy)
        d = self._dim
        x = np.zeros(d) if x0 is None else np.array(x0, dtype=np.float64)
        if x.shape != (d,):
            raise ValueError('x0 must have shape ({},); got {}'.format(d, x.shape))
        if isinstance(max_iter, bool) or int(max_iter) != max_iter or max_iter < 1:
            raise ValueError('max_iter must be a positive integer')
        if not (tol > 0):
            raise ValueError('tol must be positive')
        return newton_ascent(self._value_grad_hessian, x, int(max_iter), float(tol))


class SourceModel(DeviceModel):
    """A log density outside the built-in set, given as HIP device code -- the adaptor for what the reference
    does with an arbitrary Python callable and autograd (``viabel/models.py:17-39``,
    ``convenience.py:75`` ``bbvi(dim, log_density=...)``).

    ``source`` is HIP C++ that defines::

        __device__ double vb_log_density(const double* z, int d, const double* params, double* grad);

    returning ``f(z)`` for one sample ``z[0..d)`` and writing its gradient to ``grad[0..d)`` unless ``grad`` is
    NULL; ``params`` is the array given here (data, hyper-parameters), resident on the device.  With
    ``grad='auto'`` the source gives only the density, generic in its scalar type --
    ``template <class T> __device__ T vb_log_density(vb::vec<T> z, int d, const double* params);`` (``z[j]`` is a ``T``;
    ``+ - * /``, comparisons, ``log exp sqrt log1p expm1 pow tanh sin cos atan erf fabs fmin fmax lgamma`` work on ``T``
    and mix with ``double``; ``vb::dot(row, z, d)`` is the inner product of a ``const double*`` row with the whole sample
    as one operation -- the cheap way to write a regression's linear predictor) -- and the engine differentiates it like
    autograd does the reference's callable
    (``models.py:17-39``): forward-mode dual numbers carrying 8 derivatives in registers, ``ceil(dim / 8)`` threads
    per sample, exact to rounding.  The source is
    compiled for the GPU with hiprtc when the model is first bound; a source that does not compile raises
    ``ValueError`` with the compiler's log.  One thread evaluates one sample; a density that is a sum over data
    can have K threads per sample instead (``dim <= 128``): ``#define VB_LOG_DENSITY_PARTS K`` (a power of two up to
    64) and define ``vb_log_density_part(z, d, params, grad, part, n_parts)`` returning the share of ``f`` and adding
    the share of the gradient (``grad`` arrives zeroed) of, say, the observations ``part, part + K, ...`` with the
    prior in part 0 -- several times faster for a few hundred observations (``DESIGN.md`` 4.8).  ``ExclusiveKL`` (both estimator forms; with the mean-field families also the four RGE control variates,
    the model's Hessian terms taken as central differences of its device gradient),
    ``AlphaDivergence`` and ``DISInclusiveKL`` take it with every family; the model can be called on host samples, and ``vi_diagnostics`` forms its importance weights on the device."""

    def __init__(self, dim, source, params=None, grad='explicit'):
        if not isinstance(source, (str, bytes)) or not source:
            raise ValueError('source must be a non-empty string of HIP code')
        if grad not in ('explicit', 'auto'):
            raise ValueError("grad must be 'explicit' (the source writes the gradient) or 'auto'")
        self._source = source.encode() if isinstance(source, str) else bytes(source)
        if grad == 'auto':
            # the density alone, generic in its scalar type:
            #     template <class T> __device__ T vb_log_density(vb::vec<T> z, int d, const double* params);
            # differentiated on the device by forward-mode dual numbers, ceil(dim / 8) threads per sample
            self._source = b'#define VB_AUTO_GRAD 1\n' + self._source
        self.grad_mode = grad
        self.params = np.ascontiguousarray(np.zeros(0) if params is None else params, dtype=np.float64).ravel()
        super().__init__(dim)

    def _build_spec(self):
        return (_lib.MODEL_SOURCE, self._dim, self.params, np.zeros(0, dtype=np.int64), self._source)


class CallableModel(DeviceModel):
    """A target that exists only as a host (Python) callable -- the reference's front door ``Model(log_density)``
    (``viabel/models.py:17-39``, ``convenience.py:69-75``) and, with ``grad_log_density``, the contract of its
    ``StanModel`` (``models.py:80-104``: ``log_prob`` with ``grad_log_prob`` as its vector-Jacobian product).

    ``log_density``: ``(N, D) ndarray -> (N,)``; ``grad_log_density``: ``(N, D) -> (N, D)``.  Alternatively
    ``value_and_grad``: ``(N, D) -> ((N,), (N, D))`` in one call.  Without a gradient the engine differentiates the
    callable numerically (central differences, ``2 D`` extra calls per evaluation, relative error ~1e-9; the reference
    uses autograd, which is not available to a foreign callable here) and says so once in a ``UserWarning``.

    The estimator stays on the GPU: the engine draws the samples, hands them to the callable through pinned host
    memory (``vb_set_model_callback``), takes ``f`` and ``grad f`` back and runs the variational log density, the
    weights and every Monte-Carlo reduction on the device as for a :class:`SourceModel` -- so every objective x family
    combination a source model supports is supported.  Each evaluation contains a host round trip of ``3 N D``
    doubles plus the callable's own time; :class:`SourceModel` is the fast route."""

    def __init__(self, dim, log_density=None, grad_log_density=None, value_and_grad=None, fd_step=1e-6):
        if log_density is None and value_and_grad is None:
            raise ValueError('give log_density or value_and_grad')
        for fn in (log_density, grad_log_density, value_and_grad):
            if fn is not None and not callable(fn):
                raise TypeError('log_density / grad_log_density / value_and_grad must be callables')
        self._f, self._g, self._fg = log_density, grad_log_density, value_and_grad
        self._fd_step = float(fd_step)
        self._warned = False
        self._error = [None]
        super().__init__(dim)
        self._callback = _lib.MODEL_CALLBACK_TYPE(self._trampoline)

    # -- host evaluation ------------------------------------------------------------------------------------------
    def _values(self, z):
        f = self._f(z) if self._f is not None else self._fg(z)[0]
        f = np.asarray(f, dtype=np.float64)
        if f.shape != (z.shape[0],):
            raise ValueError('log_density returned shape {}, expected ({},)'.format(f.shape, z.shape[0]))
        return f

    def _values_and_grads(self, z):
        n, d = z.shape
        if self._fg is not None:
            f, g = self._fg(z)
        elif self._g is not None:
            f, g = self._f(z), self._g(z)
        else:
            if not self._warned:
                import warnings
                warnings.warn('CallableModel without a gradient: differentiating the callable by central differences '
                              '(2 D extra calls per evaluation); pass grad_log_density or value_and_grad, or write '
                              'the density as a SourceModel', UserWarning, stacklevel=3)
                self._warned = True
            f = self._f(z)
            h = self._fd_step * np.maximum(1.0, np.abs(z))
            g = np.empty((n, d))
            for j in range(d):                      # one batched call per coordinate and side
                zp, zm = z.copy(), z.copy()
                zp[:, j] += h[:, j]
                zm[:, j] -= h[:, j]
                g[:, j] = (np.asarray(self._f(zp), dtype=np.float64) - np.asarray(self._f(zm), dtype=np.float64)) \
                    / (zp[:, j] - zm[:, j])
        f = np.asarray(f, dtype=np.float64)
        g = np.asarray(g, dtype=np.float64)
        if f.shape != (n,) or g.shape != (n, d):
            raise ValueError('model callables returned shapes {} / {}, expected ({},) / ({}, {})'.format(
                f.shape, g.shape, n, n, d))
        return f, g

    def _trampoline(self, _user, zp, n, d, fp, gp):
        try:
            z = np.ctypeslib.as_array(zp, shape=(n, d)).copy()       # the callable may keep or modify its argument
            if gp:
                f, g = self._values_and_grads(z)
                np.ctypeslib.as_array(gp, shape=(n, d))[...] = g
            else:
                f = self._values(z)
            np.ctypeslib.as_array(fp, shape=(n,))[...] = f
            return 0
        except BaseException as exc:      # noqa: B902 -- an exception must not unwind through the C frames
            self._error[0] = exc
            return 1

    def _build_spec(self):
        empty = np.zeros(0)
        return (_lib.MODEL_SOURCE, self._dim, empty, np.zeros(0, dtype=np.int64), self._callback, self._error)

    def _refuse_ksd(self):
        raise NotImplementedError(
            'ksd_from_draws evaluates the scores on the device; a CallableModel has them on the host only. Evaluate '
            'scores = model.grad(x) and call viabel_amd.ksd(samples=x, scores=scores) (or Engine.ksd(x, scores=scores))')

    def _refuse_svgd(self, what):
        raise NotImplementedError(
            '{} evaluates the scores on the device; a CallableModel has them on the host only. Write the density as a '
            'SourceModel, or evaluate scores = model.grad(x) and call Engine.svgd_direction(x, scores=scores)'.format(what))


def as_device_model(model, dim):
    """What the objectives bind: a :class:`DeviceModel` as it is; the reference's ``Model(log_density)`` or a bare
    callable as a :class:`CallableModel` of dimension ``dim`` (gradient by central differences unless the caller
    builds the ``CallableModel`` with one)."""
    if isinstance(model, DeviceModel):
        return model
    if isinstance(model, Model):
        return CallableModel(dim, model._log_density)
    if callable(model):
        return CallableModel(dim, model)
    raise TypeError('model must be a viabel_amd device model (GaussianModel, FunnelModel, CorrelatedGaussianModel, a '
                    'regression model, SourceModel), a Model(log_density) or a callable; got %r'
                    % type(model).__name__)


class GaussianModel(DeviceModel):
    """``sum_d norm.logpdf(x_d; mean_d, stdev_d)`` -- the target of the reference's own
    objective / convenience tests (``tests/test_objectives.py:15-19``)."""

    def __init__(self, mean, stdev):
        mean = np.asarray(mean, dtype=np.float64).ravel()
        stdev = np.broadcast_to(np.asarray(stdev, dtype=np.float64).ravel(), mean.shape).copy()
        if np.any(stdev <= 0):
            raise ValueError('stdev must be positive')
        self.mean, self.stdev = mean, stdev
        super().__init__(mean.size)

    def _build_spec(self):
        return (_lib.MODEL_GAUSS_DIAG, self._dim, np.concatenate([self.mean, self.stdev]),
                np.zeros(0, dtype=np.int64))

    def hessian(self, x):
        """``-diag(1 / stdev^2)`` wherever ``x`` lies (host algebra): (D,) -> (D, D), (N, D) -> (N, D, D)."""
        x, one = self._rows(x)
        H = -np.diag(1.0 / (self.stdev * self.stdev))
        return H if one else np.repeat(H[np.newaxis], x.shape[0], axis=0)


class FunnelModel(DeviceModel):
    """D-dimensional funnel generalising ``docs/source/quickstart.ipynb:23-29``.

    Coordinate ``scale_index`` (default: the last; index 1 at D=2 as in the notebook) is the
    log-scale ``v ~ N(0, log_sigma_stdev)``; every other coordinate is ``N(0, exp(v))``.
    """

    def __init__(self, dim, scale_index=None, log_sigma_stdev=1.0):
        dim = int(dim)
        if dim < 2:
            raise ValueError('the funnel needs at least 2 dimensions')
        self.scale_index = dim - 1 if scale_index is None else int(scale_index)
        if not 0 <= self.scale_index < dim:
            raise ValueError('scale_index out of range')
        if log_sigma_stdev <= 0:
            raise ValueError('log_sigma_stdev must be positive')
        self.log_sigma_stdev = float(log_sigma_stdev)
        super().__init__(dim)

    def _build_spec(self):
        return (_lib.MODEL_FUNNEL, self._dim, np.array([self.log_sigma_stdev]),
                np.array([self.scale_index], dtype=np.int64))


class CorrelatedGaussianModel(DeviceModel):
    """``N(mean, covariance)`` with a dense covariance (target of the full-rank configs)."""

    def __init__(self, mean, covariance=None, precision=None):
        mean = np.asarray(mean, dtype=np.float64).ravel()
        if (covariance is None) == (precision is None):
            raise ValueError('give exactly one of covariance / precision')
        if precision is None:
            precision = np.linalg.inv(np.asarray(covariance, dtype=np.float64))
        precision = np.asarray(precision, dtype=np.float64)
        if precision.shape != (mean.size, mean.size):
            raise ValueError('precision must be (D, D)')
        self.mean = mean
        self.precision = 0.5 * (precision + precision.T)
        sign, self.logdet_precision = np.linalg.slogdet(self.precision)
        if sign <= 0:
            raise ValueError('precision must be positive definite')
        super().__init__(mean.size)

    def _build_spec(self):
        return (_lib.MODEL_GAUSS_FULL, self._dim,
                np.concatenate([self.mean, self.precision.ravel(), [self.logdet_precision]]),
                np.zeros(0, dtype=np.int64))

    def hessian(self, x):
        """Minus the precision matrix wherever ``x`` lies (host algebra): (D,) -> (D, D), (N, D) -> (N, D, D)."""
        x, one = self._rows(x)
        H = -self.precision
        return H.copy() if one else np.repeat(H[np.newaxis], x.shape[0], axis=0)


class LogisticRegressionModel(DeviceModel):
    """Bayesian logistic regression ``y_i ~ Bernoulli(sigmoid(x_i' b))`` with a ``N(0, prior_sd)`` prior.

    Not in the reference (BASELINE configs[4] names a logistic-regression model that the
    upstream tree does not contain); the prior scale 10 follows the Stan model of the reference's tests
    (``viabel/tests/test_models.py:41``).  Its gradient couples all coordinates through ``X``, so the engine
    evaluates it with two fp64 MFMA GEMMs per objective call.
    """

    _pointwise_entry = 'glm_pointwise'

    def __init__(self, X, y, prior_sd=10.0):
        X = np.ascontiguousarray(X, dtype=np.float64)
        y = np.asarray(y, dtype=np.float64).ravel()
        if X.ndim != 2 or y.shape != (X.shape[0],):
            raise ValueError('X must be (n_data, dim) and y (n_data,)')
        if prior_sd <= 0:
            raise ValueError('prior_sd must be positive')
        self.X, self.y, self.prior_sd = X, y, float(prior_sd)
        super().__init__(X.shape[1])

    def _build_spec(self):
        return (_lib.MODEL_LOGISTIC, self._dim, np.concatenate([self.X.ravel(), self.y, [self.prior_sd]]),
                np.array([self.X.shape[0]], dtype=np.int64))

    @property
    def n_data(self):
        return self.X.shape[0]

    def pointwise_log_likelihood(self, x):
        """``log p(y_i | x_i' theta_s)`` for every draw (row of ``x``) and observation: ``(S, n_data)``, the ``log_lik``
        argument of :func:`psisloo`.  Normalised densities (the Poisson ``- log y_i!``, the Gaussian
        ``- log noise_sd - log(2 pi) / 2`` included), without the prior; one fp64 MFMA product with the likelihood in
        its epilogue (``vb_glm_pointwise``).  ``x``: (S, D), or (D,) for one draw."""
        return self._pointwise(x)

    def predict_from_draws(self, x, X_new=None, y_new=None, log_weights=None):
        """Posterior prediction from the draws ``x`` (S, D) -- or (D,) for one -- and their log weights ``log_weights``
        (S,; None: equal weights; normalised on the way, ``-inf`` drops a draw).  ``X_new`` (m, D): the design to predict
        at, ``y_new`` (m,) held-out responses; ``X_new=None`` predicts the model's own design, ``y_new=None`` then means
        its own responses.  Returns a dict of ``(m,)`` arrays with ``eta_is = x_new_i' theta_s``: ``eta_mean``,
        ``eta_var`` (weighted mean and variance of the linear predictor), ``mean`` (of the response: sigmoid / exp /
        identity of eta, averaged), ``var`` (of the response, by the law of total variance) and -- with a response --
        ``lpd[i] = log sum_s w_s p(y_i | eta_is)`` as a normalised density.  One fp64 MFMA product and one reduction
        kernel (``vb_glm_predict``): the (m, S) matrix stays on the device, five m-vectors come back."""
        x, _ = self._rows(x)
        if X_new is not None:
            X_new = np.ascontiguousarray(X_new, dtype=np.float64)
            if X_new.ndim != 2 or X_new.shape[1] != self._dim:
                raise ValueError('X_new must have shape (m, {}); got {}'.format(self._dim, X_new.shape))
            if X_new.shape[0] < 1:
                raise ValueError('X_new must have at least one row')
        m = self.n_data if X_new is None else X_new.shape[0]
        if y_new is not None:
            y_new = np.asarray(y_new, dtype=np.float64)
            if y_new.shape != (m,):
                raise ValueError('y_new must have shape ({},); got {}'.format(m, y_new.shape))
            self._check_response(y_new)
        if log_weights is not None:
            log_weights = np.asarray(log_weights, dtype=np.float64)
            if log_weights.shape != (x.shape[0],):
                raise ValueError('log_weights must have shape ({},)'.format(x.shape[0]))
            if not np.any(np.isfinite(log_weights)):
                raise ValueError('no log weight is finite')
        eng = _lib.default_engine()
        eng.set_model(self.device_spec())
        return eng.glm_predict(x, log_w=log_weights, X_new=X_new, y_new=y_new)

    def _check_response(self, y):
        pass

    def hessian(self, x):
        """Exact Hessian ``-X' diag(w) X - I / prior_sd^2`` at each row of ``x`` (``w`` the likelihood's curvature in the
        linear predictor) from one streaming pass over the design and one fp64 MFMA Gram product on the device
        (``vb_glm_value_grad_hessian``): (D,) -> (D, D), (N, D) -> (N, D, D).  Exactly symmetric."""
        x, one = self._rows(x)
        eng = _lib.default_engine()
        eng.set_model(self.device_spec())
        out = np.empty((x.shape[0], self._dim, self._dim))
        for n, xn in enumerate(x):
            out[n] = eng.glm_value_grad_hessian(xn, True)[2]
        return out[0] if one else out

    def _value_grad_hessian(self, x, want_hessian=True):
        eng = _lib.default_engine()
        eng.set_model(self.device_spec())
        return eng.glm_value_grad_hessian(np.asarray(x, dtype=np.float64), want_hessian)


class PoissonRegressionModel(LogisticRegressionModel):
    """Bayesian Poisson regression ``y_i ~ Poisson(exp(x_i' b))`` with a ``N(0, prior_sd)`` prior: the same two-GEMM
    pipeline as the logistic target with the log link in the GEMM epilogue (not in the reference)."""

    def __init__(self, X, y, prior_sd=10.0):
        super().__init__(X, y, prior_sd)
        self._check_response(self.y)

    def _check_response(self, y):
        if np.any(y < 0):
            raise ValueError('counts must be non-negative')

    def _build_spec(self):
        return (_lib.MODEL_LOGISTIC, self._dim, np.concatenate([self.X.ravel(), self.y, [self.prior_sd]]),
                np.array([self.X.shape[0], _lib.GLM_POISSON], dtype=np.int64))


class LinearRegressionModel(LogisticRegressionModel):
    """Bayesian linear regression ``y_i ~ N(x_i' b, noise_sd)`` with a ``N(0, prior_sd)`` prior (known noise scale);
    the identity-link member of the same pipeline (not in the reference)."""

    def __init__(self, X, y, prior_sd=10.0, noise_sd=1.0):
        super().__init__(X, y, prior_sd)
        if noise_sd <= 0:
            raise ValueError('noise_sd must be positive')
        self.noise_sd = float(noise_sd)

    def _build_spec(self):
        return (_lib.MODEL_LOGISTIC, self._dim,
                np.concatenate([self.X.ravel(), self.y, [self.prior_sd, self.noise_sd]]),
                np.array([self.X.shape[0], _lib.GLM_GAUSSIAN], dtype=np.int64))


class SoftmaxRegressionModel(DeviceModel):
    """Bayesian multinomial logistic (softmax) regression ``y_i ~ Categorical(softmax(x_i' b_0, ..., x_i' b_{C-1}))``.

    ``X`` is ``(n_data, p)``, ``y`` holds integer labels in ``[0, n_classes)`` (an integer array, or a float array
    with integral values).  ``dim = n_classes * p`` and the parameter is **class-major**:
    ``theta = [b_0 | b_1 | ... | b_{C-1}]``, each ``b_c`` of length ``p``.  All ``C p`` coordinates are free and carry
    the ``N(0, prior_sd)`` prior -- no reference class is pinned: the likelihood is invariant under adding one vector
    to every ``b_c`` and the prior alone fixes that direction, so compare fits through the differences
    ``b_c - b_0``.  For ``C = 2`` the likelihood equals the logistic one at ``beta = b_1 - b_0``.  There is no
    intercept: add a column of ones to ``X``.  Log density, normalised in ``theta``::

        eta_ic   = x_i' b_c
        f(theta) = sum_i [eta_{i, y_i} - logsumexp_c eta_ic] - |theta|^2 / (2 sd^2) - C p (log sd + log(2 pi) / 2)
        df/db_c  = sum_i ([y_i = c] - softmax_c(eta_i)) x_i - b_c / sd^2

    The classes of an observation are coupled, so this is not an epilogue of one GEMM: the engine packs the class
    blocks of every sample as rows, forms all predictors with one fp64 MFMA product, runs a coupling kernel
    (max-subtracted logsumexp, residuals in place) and takes the gradient with the regression targets' second product
    (``csrc/vb_softmax.hip``, ``DESIGN.md``).  To every objective it looks like a :class:`SourceModel` -- per-sample
    ``f`` and gradient formed before the streaming pass -- and is accepted wherever one is: ``ExclusiveKL`` (both
    estimator forms, the RGE control variates, ``NVPFlow``), ``AlphaDivergence`` and ``DISInclusiveKL`` with every
    family, ``bbvi``, ``vi_diagnostics`` and the device-resident fit.  Not in the reference."""

    _pointwise_entry = 'softmax_pointwise'

    def __init__(self, X, y, n_classes, prior_sd=10.0):
        X = np.ascontiguousarray(X, dtype=np.float64)
        y_in = np.asarray(y)
        if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1 or y_in.shape != (X.shape[0],):
            raise ValueError('X must be (n_data, p) and y (n_data,)')
        if isinstance(n_classes, bool) or int(n_classes) != n_classes or int(n_classes) < 2:
            raise ValueError('n_classes must be an integer >= 2')
        n_classes = int(n_classes)
        if y_in.dtype.kind not in 'iuf':
            raise ValueError('y must hold integer labels (an integer array, or floats with integral values)')
        y = y_in.astype(np.float64)
        if not np.all(np.isfinite(y)) or np.any(y != np.floor(y)):
            raise ValueError('y must hold integral labels')
        if np.any(y < 0) or np.any(y >= n_classes):
            raise ValueError('labels must lie in [0, n_classes)')
        if not prior_sd > 0:
            raise ValueError('prior_sd must be positive')
        self.X, self.y, self.prior_sd = X, y, float(prior_sd)
        self._n_classes = n_classes
        super().__init__(n_classes * X.shape[1])

    def _build_spec(self):
        return (_lib.MODEL_SOFTMAX, self._dim, np.concatenate([self.X.ravel(), self.y, [self.prior_sd]]),
                np.array([self.X.shape[0], self._n_classes], dtype=np.int64))

    @property
    def n_data(self):
        return self.X.shape[0]

    @property
    def n_classes(self):
        return self._n_classes

    def pointwise_log_likelihood(self, x):
        """``log p(y_i | theta_s) = eta_{i, y_i} - logsumexp_c eta_ic`` for every draw (row of ``x``) and observation:
        ``(S, n_data)``, the ``log_lik`` argument of :func:`psisloo` (``psisloo(log_lik, log_ratios)`` is this model's
        route to LOO; ``loo()`` takes the one-predictor regression targets only).  Without the prior
        (``vb_softmax_pointwise``).  ``x``: (S, D), or (D,) for one draw."""
        return self._pointwise(x)


# the one-predictor GLM likelihoods of the multilevel and the sparse target, and what each asks of the response
_GLM_LINKS = {'logistic': _lib.GLM_BERNOULLI_LOGIT, 'poisson': _lib.GLM_POISSON, 'gaussian': _lib.GLM_GAUSSIAN}


def _check_glm_response(likelihood, y):
    if not np.all(np.isfinite(y)):
        raise ValueError('y must be finite')
    if likelihood == 'logistic' and np.any((y != 0) & (y != 1)):
        raise ValueError('y must lie in {0, 1}')
    if likelihood == 'poisson' and np.any(y < 0):
        raise ValueError('counts must be non-negative')


class MultilevelRegressionModel(DeviceModel):
    """A varying-intercept (multilevel) GLM: ``eta_i = x_i' b + a_{g_i}`` with group effects ``a_j ~ N(0, tau)`` whose
    scale ``tau`` is itself a parameter -- the hierarchical posterior with funnel geometry that ``vi_diagnostics`` exists
    to expose.

    ``X`` is ``(n_data, p)``, ``groups`` holds integer labels in ``[0, n_groups)`` (an integer array, or a float array
    with integral values; groups without observations are legal), ``likelihood`` is ``'logistic'`` (``y`` in
    ``{0, 1}``), ``'poisson'`` (``y >= 0``) or ``'gaussian'`` (known ``noise_sd``).  The parameter is non-centred and
    unconstrained, ``dim = p + n_groups + 1``::

        theta    = [ b (p) | u (J) | omega ],   tau = exp(omega),   group effects a = tau * u
        eta_i    = x_i' b + tau * u_{g_i}
        f(theta) = sum_i log p(y_i | eta_i)                             normalised, as the flat regression targets have it
                   - |b|^2 / (2 prior_sd^2) - p (log prior_sd + log(2 pi) / 2)          b ~ N(0, prior_sd)
                   - |u|^2 / 2 - J log(2 pi) / 2                                        u ~ N(0, 1)
                   + log 2 - log tau_sd - log(2 pi) / 2 - tau^2 / (2 tau_sd^2) + omega  tau ~ HalfNormal(tau_sd), Jacobian
        df/db    = X' r - b / prior_sd^2,   r_i = d log p(y_i | eta_i) / d eta_i
        df/du_j  = tau * sum_{i: g_i = j} r_i - u_j
        df/domega= tau * sum_i r_i u_{g_i} - tau^2 / tau_sd^2 + 1

    There is no intercept: add a column of ones to ``X``.  The constructor sorts the observations by group (stably) so
    that the device sees contiguous group runs; :meth:`pointwise_log_likelihood` answers in the caller's order.  The
    engine forms all predictors with one fp64 MFMA product, applies the link in a kernel of its own, takes the coefficient
    gradient with the regression targets' second product and the group gradients by segmented sums
    (``csrc/vb_multilevel.hip``, ``DESIGN.md`` 4.16).  To every objective it looks like a :class:`SourceModel` and is
    accepted wherever one is: ``ExclusiveKL`` (both estimator forms, the RGE control variates, ``NVPFlow``),
    ``AlphaDivergence`` and ``DISInclusiveKL`` with every family, ``bbvi``, ``vi_diagnostics`` and the device-resident
    fit.  Not in the reference."""

    _LINKS = _GLM_LINKS
    _pointwise_entry = 'multilevel_pointwise'

    def __init__(self, X, y, groups, n_groups, likelihood='logistic', prior_sd=10.0, tau_sd=1.0, noise_sd=1.0):
        X = np.ascontiguousarray(X, dtype=np.float64)
        y = np.asarray(y, dtype=np.float64)
        g_in = np.asarray(groups)
        if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1 or y.shape != (X.shape[0],) or g_in.shape != (X.shape[0],):
            raise ValueError('X must be (n_data, p) with p >= 1, y and groups (n_data,)')
        if isinstance(n_groups, bool) or int(n_groups) != n_groups or int(n_groups) < 1:
            raise ValueError('n_groups must be an integer >= 1')
        n_groups = int(n_groups)
        if g_in.dtype.kind not in 'iuf':
            raise ValueError('groups must hold integer labels (an integer array, or floats with integral values)')
        g = g_in.astype(np.float64)
        if not np.all(np.isfinite(g)) or np.any(g != np.floor(g)):
            raise ValueError('groups must hold integral labels')
        if np.any(g < 0) or np.any(g >= n_groups):
            raise ValueError('group labels must lie in [0, n_groups)')
        if likelihood not in self._LINKS:
            raise ValueError("likelihood must be 'logistic', 'poisson' or 'gaussian'")
        if not prior_sd > 0 or not tau_sd > 0 or not noise_sd > 0:
            raise ValueError('prior_sd, tau_sd and noise_sd must be positive')
        _check_glm_response(likelihood, y)
        g = g.astype(np.int64)
        # contiguous group runs for the device: a stable sort, undone by pointwise_log_likelihood
        self.perm = np.argsort(g, kind='stable')
        self.X, self.y, self.groups = np.ascontiguousarray(X[self.perm]), y[self.perm], g[self.perm]
        self.offsets = np.concatenate([[0], np.cumsum(np.bincount(g, minlength=n_groups))]).astype(np.int64)
        self.likelihood = likelihood
        self.prior_sd, self.tau_sd, self.noise_sd = float(prior_sd), float(tau_sd), float(noise_sd)
        self._n_groups = n_groups
        super().__init__(X.shape[1] + n_groups + 1)

    def _build_spec(self):
        return (_lib.MODEL_MULTILEVEL, self._dim,
                np.concatenate([self.X.ravel(), self.y, [self.prior_sd, self.tau_sd, self.noise_sd]]),
                np.concatenate([[self.n_data, self._n_groups, self._LINKS[self.likelihood]], self.offsets,
                                self.groups]).astype(np.int64))

    @property
    def n_data(self):
        return self.X.shape[0]

    @property
    def n_groups(self):
        return self._n_groups

    @property
    def n_features(self):
        return self.X.shape[1]

    def unpack(self, theta):
        """``(b, u, tau)`` of ``theta`` ``(D,)`` or ``(N, D)``; the group effects are ``tau[..., None] * u``."""
        theta = np.asarray(theta, dtype=np.float64)
        if theta.ndim not in (1, 2) or theta.shape[-1] != self._dim:
            raise ValueError('theta must have shape (N, {0}) or ({0},)'.format(self._dim))
        p = self.n_features
        return theta[..., :p], theta[..., p:p + self._n_groups], np.exp(theta[..., -1])

    def pointwise_log_likelihood(self, x):
        """``log p(y_i | x_i' b_s + tau_s u_{s, g_i})`` for every draw (row of ``x``) and observation, in the order the
        observations were given to the constructor: ``(S, n_data)``, the ``log_lik`` argument of :func:`psisloo`
        (``psisloo(log_lik, log_ratios)`` is this model's route to LOO).  Normalised densities, without the priors
        (``vb_multilevel_pointwise``).  ``x``: (S, D), or (D,) for one draw."""
        return self._pointwise(x)

    def _pointwise_order(self, out):
        back = np.empty_like(out)
        back[:, self.perm] = out
        return back


class LocationScaleRegressionModel(DeviceModel):
    """Location-scale regression: the mean AND the log-scale of every observation are linear in the parameter -- linear
    regression with an unknown noise scale (``W=None``), heteroscedastic regression (a scale design ``W``) and, with
    ``likelihood='student_t'``, the robust regression of the reference's ``docs/source/robust-regression.ipynb``.

    ``X`` is ``(n_data, p)``, ``W`` is ``(n_data, q)`` or ``None``, ``likelihood`` is ``'gaussian'`` or ``'student_t'``
    (``df > 0`` fixed, used by ``'student_t'`` only).  The parameter is unconstrained, ``dim = p + q``, no Jacobian::

        theta    = [ b (p) | g (q) ]
        eta_i    = x_i' b,   s_i = w_i' g,   sigma_i = exp(s_i),   z_i = (y_i - eta_i) exp(-s_i)
        gaussian : l_i = -s_i - z_i^2 / 2 - log(2 pi) / 2
        student_t: l_i = c(nu) - s_i - (nu + 1) / 2 log1p(z_i^2 / nu),
                   c(nu) = lgamma((nu + 1) / 2) - lgamma(nu / 2) - log(nu pi) / 2
        f(theta) = sum_i l_i - |b|^2 / (2 prior_sd^2)       - p (log prior_sd       + log(2 pi) / 2)
                             - |g|^2 / (2 scale_prior_sd^2) - q (log scale_prior_sd + log(2 pi) / 2)

    With ``W=None`` the scale is one constant: ``q = 1``, ``s_i = g_0``, so ``theta[-1] = log sigma`` under a log-normal
    prior ``log sigma ~ N(0, scale_prior_sd)``; this case does not pay for a second design matrix.  There is no intercept
    in either predictor: add a column of ones to ``X`` (and to ``W``).  The engine forms both predictors with fp64 MFMA
    products, applies the likelihood in a link kernel and takes both gradient blocks with the regression targets' second
    product (``csrc/vb_locscale.hip``, ``DESIGN.md`` 4.17).  To every objective it looks like a :class:`SourceModel` and is
    accepted wherever one is: ``ExclusiveKL`` (both estimator forms, the RGE control variates, ``NVPFlow``),
    ``AlphaDivergence`` and ``DISInclusiveKL`` with every family, ``bbvi``, ``vi_diagnostics`` and the device-resident
    fit.  ``loo()`` takes the one-predictor regression targets only: this model's route to LOO is
    ``psisloo(model.pointwise_log_likelihood(x), log_ratios)``.  Not in the reference as a model class."""

    _LIKELIHOODS = {'gaussian': _lib.LOCSCALE_GAUSSIAN, 'student_t': _lib.LOCSCALE_STUDENT_T}
    _pointwise_entry = 'locscale_pointwise'

    def __init__(self, X, y, W=None, likelihood='gaussian', df=4.0, prior_sd=10.0, scale_prior_sd=1.0):
        X = np.ascontiguousarray(X, dtype=np.float64)
        y = np.asarray(y, dtype=np.float64)
        if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1 or y.shape != (X.shape[0],):
            raise ValueError('X must be (n_data, p) with p >= 1 and y (n_data,)')
        if W is not None:
            W = np.ascontiguousarray(W, dtype=np.float64)
            if W.ndim != 2 or W.shape[0] != X.shape[0] or W.shape[1] < 1:
                raise ValueError('W must be (n_data, q) with q >= 1, or None for a constant scale')
            if not np.all(np.isfinite(W)):
                raise ValueError('W must be finite')
        if likelihood not in self._LIKELIHOODS:
            raise ValueError("likelihood must be 'gaussian' or 'student_t'")
        if not prior_sd > 0 or not scale_prior_sd > 0:
            raise ValueError('prior_sd and scale_prior_sd must be positive')
        if not df > 0 or not np.isfinite(df):
            raise ValueError('df must be positive and finite')
        if not np.all(np.isfinite(y)) or not np.all(np.isfinite(X)):
            raise ValueError('X and y must be finite')
        self.X, self.y, self.W = X, y, W
        self.likelihood, self.df = likelihood, float(df)
        self.prior_sd, self.scale_prior_sd = float(prior_sd), float(scale_prior_sd)
        super().__init__(X.shape[1] + (1 if W is None else W.shape[1]))

    def _build_spec(self):
        w = np.zeros(0) if self.W is None else self.W.ravel()
        return (_lib.MODEL_LOCSCALE, self._dim,
                np.concatenate([self.X.ravel(), self.y, w, [self.prior_sd, self.scale_prior_sd, self.df]]),
                np.array([self.n_data, self.n_features, self.n_scale_features, self._LIKELIHOODS[self.likelihood],
                          1 if self.W is None else 0], dtype=np.int64))

    @property
    def n_data(self):
        return self.X.shape[0]

    @property
    def n_features(self):
        return self.X.shape[1]

    @property
    def n_scale_features(self):
        return 1 if self.W is None else self.W.shape[1]

    def unpack(self, theta):
        """``(b, g)`` of ``theta`` ``(D,)`` or ``(N, D)``."""
        theta = np.asarray(theta, dtype=np.float64)
        if theta.ndim not in (1, 2) or theta.shape[-1] != self._dim:
            raise ValueError('theta must have shape (N, {0}) or ({0},)'.format(self._dim))
        p = self.n_features
        return theta[..., :p], theta[..., p:]

    def sigma(self, theta):
        """The per-observation scales ``exp(W g)`` at ``theta``: ``(n_data,)`` for ``(D,)``, ``(N, n_data)`` for ``(N, D)``
        (evaluated on the host)."""
        g = self.unpack(theta)[1]
        if self.W is None:
            return np.exp(g) * np.ones(self.n_data)
        return np.exp(g @ self.W.T)

    def pointwise_log_likelihood(self, x):
        """The normalised terms ``l_i`` for every draw (row of ``x``) and observation: ``(S, n_data)``, the ``log_lik``
        argument of :func:`psisloo` (``psisloo(log_lik, log_ratios)`` is this model's route to LOO).  Without the priors
        (``vb_locscale_pointwise``).  ``x``: (S, D), or (D,) for one draw."""
        return self._pointwise(x)


def _canonical_csr(data, indices, indptr, n_rows, n_cols):
    """Validate a CSR triple and return it canonical: indices sorted within each row, duplicates summed in input order,
    entries that are exactly 0 after summing dropped.  ``(data float64, indices int32, indptr int64)``."""
    data = np.asarray(data, dtype=np.float64).ravel()
    indices_in, indptr_in = np.asarray(indices).ravel(), np.asarray(indptr).ravel()
    if indices_in.dtype.kind not in 'iu' and indices_in.size or indptr_in.dtype.kind not in 'iu':
        raise ValueError('indices and indptr must be integer arrays')
    indices, indptr = indices_in.astype(np.int64), indptr_in.astype(np.int64)
    if n_rows < 1 or n_cols < 1:
        raise ValueError('the design must have at least one row and one column')
    if n_rows >= 2 ** 31 or n_cols >= 2 ** 31 or data.size >= 2 ** 31:
        raise ValueError('n_data, p and nnz must be below 2^31')
    if indptr.shape != (n_rows + 1,):
        raise ValueError('indptr must have n_data + 1 = {} entries; got {}'.format(n_rows + 1, indptr.size))
    if data.shape != indices.shape:
        raise ValueError('data and indices must have the same length')
    if indptr[0] != 0 or indptr[-1] != data.size or np.any(np.diff(indptr) < 0):
        raise ValueError('indptr must be monotone from 0 to nnz = {}'.format(data.size))
    if not np.all(np.isfinite(data)):
        raise ValueError('the design must be finite')
    if indices.size and (indices.min() < 0 or indices.max() >= n_cols):
        raise ValueError('column indices must lie in [0, {})'.format(n_cols))
    rows = np.repeat(np.arange(n_rows, dtype=np.int64), np.diff(indptr))
    order = np.lexsort((indices, rows))                  # stable: duplicates keep their input order
    rows, cols, vals = rows[order], indices[order], data[order]
    first = np.ones(vals.size, dtype=bool)
    first[1:] = (rows[1:] != rows[:-1]) | (cols[1:] != cols[:-1])
    summed = np.zeros(int(np.count_nonzero(first)))
    np.add.at(summed, np.cumsum(first) - 1, vals)        # unbuffered: one addition after the other, in order
    rows, cols = rows[first], cols[first]
    keep = summed != 0.0
    rows, cols, summed = rows[keep], cols[keep], summed[keep]
    ptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n_rows))]).astype(np.int64)
    return np.ascontiguousarray(summed), cols.astype(np.int32), ptr


class SparseRegressionModel(DeviceModel):
    """Bayesian GLM ``y_i ~ p(. | x_i' theta)`` with a ``N(0, prior_sd)`` prior on a SPARSE design matrix: one-hot factors,
    interaction dummies, bag-of-words counts, hashed features.  ``likelihood`` is ``'logistic'`` (``y`` in ``{0, 1}``),
    ``'poisson'`` (``y >= 0``) or ``'gaussian'`` (known ``noise_sd``); ``dim = p``.  The density is exactly the one of
    :class:`LogisticRegressionModel`, :class:`PoissonRegressionModel` and :class:`LinearRegressionModel` on
    ``model.to_dense()``, normalised the same way::

        f(theta) = sum_i log p(y_i | x_i' theta) - |theta|^2 / (2 prior_sd^2) - p (log prior_sd + log(2 pi) / 2)

    (the Poisson ``- log y_i!`` and the Gaussian ``- log noise_sd - log(2 pi) / 2`` included), but the device holds only the
    non-zeros -- a design with 200 000 rows, 50 000 columns and ten entries per row is 2 M numbers, not 160 GB.

    ``X`` is anything with a ``.tocsr()`` method (a ``scipy.sparse`` matrix or array; the package itself does not import
    scipy), or a CSR triple ``(data, indices, indptr)`` together with ``shape=(n_data, p)``.  A dense array is refused: use
    :meth:`from_dense` (zeros dropped; for tests and small problems) or the dense classes.  The input is made canonical on
    the host: indices sorted within each row, duplicates summed in input order, entries that are exactly 0 dropped.
    ``model.csr = (data float64, indices int32, indptr int64)``; ``model.csc`` is the same matrix as the CSR of ``X'``
    (every column lists its entries in increasing observation order).  Empty rows (``eta_i = 0``) and empty columns (prior
    only) are legal.  There is no intercept: add a column of ones.

    The engine transposes each chunk of samples, forms the predictors with a gather kernel over the CSR arrays, applies the
    link, and takes the gradient with the same kernel over the CSC arrays; rows and columns longer than
    ``_lib.SPARSE_SEGMENT`` entries (an intercept) are cut into segments summed by separate waves (``csrc/vb_sparse.hip``,
    ``DESIGN.md`` 4.19).  No atomics: two calls return the same bits.  To every objective it looks like a
    :class:`SourceModel` and is accepted wherever one is: ``ExclusiveKL`` (both estimator forms, the RGE control variates,
    ``NVPFlow``), ``AlphaDivergence`` and ``DISInclusiveKL`` with every family, ``bbvi``, ``vi_diagnostics`` and the
    device-resident fit.  ``loo()`` and ``predict()`` take the dense one-predictor regression targets only: this model's
    route to LOO is ``psisloo(model.pointwise_log_likelihood(x), log_ratios)``.  Not in the reference."""

    _LINKS = _GLM_LINKS
    _pointwise_entry = 'sparse_glm_pointwise'

    def __init__(self, X, y, likelihood='logistic', prior_sd=10.0, noise_sd=1.0, shape=None):
        if hasattr(X, 'tocsr'):
            X = X.tocsr()
            if shape is not None and tuple(shape) != tuple(X.shape):
                raise ValueError('shape {} does not match the matrix ({})'.format(tuple(shape), tuple(X.shape)))
            data, indices, indptr, shape = X.data, X.indices, X.indptr, X.shape
        elif isinstance(X, (tuple, list)) and len(X) == 3 and shape is not None:
            data, indices, indptr = X
        else:
            raise ValueError('X must be a sparse matrix (anything with .tocsr()) or a CSR triple (data, indices, indptr) with '
                             'shape=(n_data, p); for a dense array use SparseRegressionModel.from_dense, or the dense classes '
                             'LogisticRegressionModel, PoissonRegressionModel and LinearRegressionModel')
        if len(shape) != 2 or int(shape[0]) != shape[0] or int(shape[1]) != shape[1]:
            raise ValueError('shape must be (n_data, p)')
        n_data, p = int(shape[0]), int(shape[1])
        if likelihood not in self._LINKS:
            raise ValueError("likelihood must be 'logistic', 'poisson' or 'gaussian'")
        if not prior_sd > 0 or not noise_sd > 0:
            raise ValueError('prior_sd and noise_sd must be positive')
        self.csr = _canonical_csr(data, indices, indptr, n_data, p)
        y = np.asarray(y, dtype=np.float64)
        if y.shape != (n_data,):
            raise ValueError('y must have shape ({},); got {}'.format(n_data, y.shape))
        _check_glm_response(likelihood, y)
        vals, cols, ptr = self.csr
        rows = np.repeat(np.arange(n_data, dtype=np.int64), np.diff(ptr))
        order = np.argsort(cols, kind='stable')          # row-major input: rows increase within every column
        self.csc = (np.ascontiguousarray(vals[order]), rows[order].astype(np.int32),
                    np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=p))]).astype(np.int64))
        self.y, self.likelihood = y, likelihood
        self.prior_sd, self.noise_sd = float(prior_sd), float(noise_sd)
        self._n_data = n_data
        super().__init__(p)

    @classmethod
    def from_dense(cls, X, y, likelihood='logistic', prior_sd=10.0, noise_sd=1.0):
        """The model of a dense ``(n_data, p)`` array, its zeros dropped (for tests and small problems)."""
        X = np.asarray(X, dtype=np.float64)
        if X.ndim != 2:
            raise ValueError('X must be (n_data, p)')
        rows, cols = np.nonzero(X)                        # row-major order
        ptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=X.shape[0]))]).astype(np.int64)
        return cls((X[rows, cols], cols, ptr), y, likelihood=likelihood, prior_sd=prior_sd, noise_sd=noise_sd, shape=X.shape)

    def _build_spec(self):
        (v, c, ptr), (vt, r, ptr_t) = self.csr, self.csc
        return (_lib.MODEL_SPARSE_GLM, self._dim, np.concatenate([v, vt, self.y, [self.prior_sd, self.noise_sd]]),
                np.concatenate([[self._n_data, self._dim, self._LINKS[self.likelihood], v.size], ptr, c, ptr_t,
                                r]).astype(np.int64))

    @property
    def n_data(self):
        return self._n_data

    @property
    def n_features(self):
        return self._dim

    @property
    def nnz(self):
        return int(self.csr[0].size)

    def to_dense(self):
        """The design as a dense ``(n_data, p)`` array (meant for small models)."""
        vals, cols, ptr = self.csr
        X = np.zeros((self._n_data, self._dim))
        X[np.repeat(np.arange(self._n_data), np.diff(ptr)), cols] = vals
        return X

    def pointwise_log_likelihood(self, x):
        """``log p(y_i | x_i' theta_s)`` for every draw (row of ``x``) and observation: ``(S, n_data)``, the ``log_lik``
        argument of :func:`psisloo` (``psisloo(log_lik, log_ratios)`` is this model's route to LOO).  Normalised densities,
        without the prior (``vb_sparse_glm_pointwise``).  ``x``: (S, D), or (D,) for one draw."""
        return self._pointwise(x)


class NeuralNetRegressionModel(DeviceModel):
    """A Bayesian neural network with one hidden layer of ``tanh`` units: a regression that is not linear in its
    predictor, and the large-dimension target for the mean-field, ``LRGaussian`` and ``NVPFlow`` families.

    ``X`` is ``(n_data, p)``, ``n_hidden = h >= 1``, ``likelihood`` is ``'gaussian'`` (known ``noise_sd``, read by this
    likelihood only), ``'logistic'`` (``y`` in ``{0, 1}``) or ``'poisson'`` (``y >= 0``).  The parameter is
    **unit-major**, ``dim = h (p + 2) + 1``, every coordinate under a ``N(0, prior_sd)`` prior::

        theta    = [ w_0 | ... | w_{h-1} | a (h) | v (h) | c ]      w_k of length p
        t_ik     = tanh(x_i' w_k + a_k)
        eta_i    = c + sum_k v_k t_ik
        f(theta) = sum_i log p(y_i | eta_i) - |theta|^2 / (2 sd^2) - dim (log sd + log(2 pi) / 2)
        r_i      = d log p(y_i | eta_i) / d eta,      delta_ik = r_i v_k (1 - t_ik^2)
        df/dc    = sum_i r_i          - c   / sd^2
        df/dv_k  = sum_i r_i t_ik     - v_k / sd^2
        df/da_k  = sum_i delta_ik     - a_k / sd^2
        df/dw_k  = sum_i delta_ik x_i - w_k / sd^2

    ``log p(y | eta)`` is a normalised density, as the flat regression targets have it.  The inputs are taken as they
    are: no standardisation and no intercept column (``a`` and ``c`` are the network's own biases); standardise ``X``
    yourself.  The posterior is invariant under permuting the hidden units and under flipping the sign of a unit's
    ``(w_k, a_k, v_k)``: compare fits through predictions, not coordinates.

    The engine takes the units of a sample as ``h`` rows of a packed matrix, forms all pre-activations with one fp64 MFMA
    product, runs a forward kernel (``tanh``, the output, the likelihood and its residual) and a backward kernel (the
    ``a`` and ``v`` sums, ``delta`` in place) and takes the weight gradient with the regression targets' second product
    (``csrc/vb_neuralnet.hip``, ``DESIGN.md`` 4.24).  To every objective it looks like a :class:`SourceModel` and is
    accepted wherever one is: ``ExclusiveKL`` (both estimator forms, the RGE control variates, ``NVPFlow``),
    ``AlphaDivergence`` and ``DISInclusiveKL`` with every family, ``bbvi``, ``vi_diagnostics``, the device-resident fit,
    ``hmc`` and the difference route of ``hessian()``.  :func:`predict` takes it (:meth:`predict_from_draws`).  ``loo()``
    takes the one-predictor regression targets only: this model's route to LOO is
    ``psisloo(model.pointwise_log_likelihood(draws), log_ratios)``.  Not in the reference."""

    _LINKS = _GLM_LINKS
    _pointwise_entry = 'nn_pointwise'

    def __init__(self, X, y, n_hidden, likelihood='gaussian', prior_sd=1.0, noise_sd=1.0):
        X = np.ascontiguousarray(X, dtype=np.float64)
        y = np.asarray(y, dtype=np.float64)
        if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1 or y.shape != (X.shape[0],):
            raise ValueError('X must be (n_data, p) with p >= 1 and y (n_data,)')
        if isinstance(n_hidden, bool) or int(n_hidden) != n_hidden or int(n_hidden) < 1:
            raise ValueError('n_hidden must be an integer >= 1')
        if likelihood not in self._LINKS:
            raise ValueError("likelihood must be 'gaussian', 'logistic' or 'poisson'")
        if not prior_sd > 0 or not noise_sd > 0:
            raise ValueError('prior_sd and noise_sd must be positive')
        if not np.all(np.isfinite(X)):
            raise ValueError('X must be finite')
        _check_glm_response(likelihood, y)
        self.X, self.y = X, y
        self.likelihood = likelihood
        self.prior_sd, self.noise_sd = float(prior_sd), float(noise_sd)
        self._n_hidden = int(n_hidden)
        super().__init__(self._n_hidden * (X.shape[1] + 2) + 1)

    def _build_spec(self):
        return (_lib.MODEL_NEURALNET, self._dim,
                np.concatenate([self.X.ravel(), self.y, [self.prior_sd, self.noise_sd]]),
                np.array([self.n_data, self._n_hidden, self._LINKS[self.likelihood]], dtype=np.int64))

    @property
    def n_data(self):
        return self.X.shape[0]

    @property
    def n_hidden(self):
        return self._n_hidden

    @property
    def n_features(self):
        return self.X.shape[1]

    def unpack(self, theta):
        """``(W, a, v, c)`` of ``theta`` ``(D,)`` or ``(N, D)``: the hidden weights ``W`` ``(..., h, p)`` (row ``k`` is
        ``w_k``), the hidden biases ``a`` and the output weights ``v`` ``(..., h)``, the output bias ``c`` ``(...)``."""
        theta = np.asarray(theta, dtype=np.float64)
        if theta.ndim not in (1, 2) or theta.shape[-1] != self._dim:
            raise ValueError('theta must have shape (N, {0}) or ({0},)'.format(self._dim))
        h, p = self._n_hidden, self.n_features
        return (theta[..., :h * p].reshape(theta.shape[:-1] + (h, p)), theta[..., h * p:h * p + h],
                theta[..., h * p + h:h * p + 2 * h], theta[..., -1])

    def pointwise_log_likelihood(self, x):
        """``log p(y_i | eta_i(theta_s))`` for every draw (row of ``x``) and observation: ``(S, n_data)``, the ``log_lik``
        argument of :func:`psisloo` (``psisloo(log_lik, log_ratios)`` is this model's route to LOO).  Normalised
        densities, without the prior (``vb_nn_pointwise``).  ``x``: (S, D), or (D,) for one draw."""
        return self._pointwise(x)

    def predict_from_draws(self, x, X_new=None, y_new=None, log_weights=None):
        """Posterior prediction from the draws ``x`` (S, D) -- or (D,) for one -- and their log weights ``log_weights``
        (S,; None: equal weights; normalised on the way, ``-inf`` drops a draw): the arguments and the returned dict of
        :meth:`LogisticRegressionModel.predict_from_draws`, with ``X_new`` ``(m, p)`` and ``eta_is`` the network's output
        of draw ``s`` at row ``i``.  One fp64 MFMA product per chunk of observations, a forward kernel and the regression
        targets' reduction kernel (``vb_nn_predict``): the (m, S) matrix stays on the device, five m-vectors come back."""
        x, _ = self._rows(x)
        p = self.n_features
        if X_new is not None:
            X_new = np.ascontiguousarray(X_new, dtype=np.float64)
            if X_new.ndim != 2 or X_new.shape[1] != p:
                raise ValueError('X_new must have shape (m, {}); got {}'.format(p, X_new.shape))
            if X_new.shape[0] < 1:
                raise ValueError('X_new must have at least one row')
        m = self.n_data if X_new is None else X_new.shape[0]
        if y_new is not None:
            y_new = np.asarray(y_new, dtype=np.float64)
            if y_new.shape != (m,):
                raise ValueError('y_new must have shape ({},); got {}'.format(m, y_new.shape))
            _check_glm_response(self.likelihood, y_new)
        if log_weights is not None:
            log_weights = np.asarray(log_weights, dtype=np.float64)
            if log_weights.shape != (x.shape[0],):
                raise ValueError('log_weights must have shape ({},)'.format(x.shape[0]))
            if not np.any(np.isfinite(log_weights)):
                raise ValueError('no log weight is finite')
        eng = _lib.default_engine()
        eng.set_model(self.device_spec())
        return eng.nn_predict(x, p, log_w=log_weights, X_new=X_new, y_new=y_new)


_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def _philox4x32_10_word0(c0, c1, c2, c3, k0, k1):
    """Word 0 of Philox4x32-10 (Salmon et al., SC'11) on uint64 arrays holding 32-bit words: the generator of
    ``csrc/vb_rng.h``, restated on the host for :meth:`MinibatchRegressionModel.batch_indices`."""
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _M32 for c in (c0, c1, c2, c3))
    for r in range(10):
        p0, p1 = m0 * c0, m1 * c2                       # 32 x 32 -> 64: no overflow in uint64
        ka = np.uint64((k0 + 0x9E3779B9 * r) & 0xFFFFFFFF)
        kb = np.uint64((k1 + 0xBB67AE85 * r) & 0xFFFFFFFF)
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ ka, p1 & _M32, (p0 >> _S32) ^ c3 ^ kb, p0 & _M32
    return c0


def refuse_minibatch(model, what):
    """``NotImplementedError`` when ``model`` is a :class:`MinibatchRegressionModel`: ``what`` needs one fixed density."""
    if isinstance(model, MinibatchRegressionModel):
        raise NotImplementedError(
            '{} needs one fixed log density; a MinibatchRegressionModel is a different density for every batch. Use '
            'model.full_model(), the same data as a full-batch target'.format(what))


class MinibatchRegressionModel(DeviceModel):
    """The flat regression targets (:class:`LogisticRegressionModel`, :class:`PoissonRegressionModel`,
    :class:`LinearRegressionModel`) evaluated on a random batch of ``batch_size`` of the ``n_data`` observations, the
    likelihood scaled by ``n_data / batch_size``: doubly stochastic variational inference, whose cost per iteration does
    not depend on ``n_data``.  ``likelihood`` is ``'logistic'`` (``y`` in ``{0, 1}``), ``'poisson'`` (``y >= 0``) or
    ``'gaussian'`` (known ``noise_sd``); ``dim = p``.  Batch number ``t`` is the density::

        f_t(theta) = (n_data / B) sum_{j in batch t} log p(y_j | x_j' theta)        without the likelihood's constants
                     - |theta|^2 / (2 prior_sd^2) - p (log prior_sd + log(2 pi) / 2)
                     + C                                the constants of ALL n_data observations, as the dense targets have

    so that ``B = n_data`` gives ``full_model()``'s density and the mean of ``f_t`` over the batches of an epoch is
    ``full_model()``'s exactly when ``B`` divides ``n_data``.  The batch is a pure function of ``(seed, t)``: batch ``t``
    owns the positions ``t B .. t B + B - 1`` of an endless stream, position ``q`` is slot ``q mod n_data`` of epoch
    ``q div n_data`` (a batch may straddle two epochs), and the slot's observation is the slot itself
    (``order='sequential'``) or its image under a keyed permutation of the epoch (``order='shuffle'``: a 6-round Feistel
    network over Philox, cycle-walked; ``DESIGN.md`` 4.23) -- every observation appears exactly once per epoch.
    :meth:`batch_indices` restates it on the host.

    ``model.batch`` is the number of the batch that ``model(x)``, ``model.grad(x)``, ``check_gradient`` and
    ``pointwise_log_likelihood`` evaluate; they do not advance it.  One ``ExclusiveKL`` call uses one batch for everything
    it evaluates and advances the counter by one; a device-resident fit advances it once per iteration.  The counter is
    the model object's: models interleaved on one engine each keep their own sequence.

    The device holds ``X`` once (no transpose).  Per evaluation an index kernel and a gather kernel form the batch's design
    in both layouts, then the two fp64 MFMA products of the dense target run on ``B`` observations
    (``csrc/vb_minibatch.hip``).  Taken by ``ExclusiveKL`` (both estimator forms) with every family, through ``bbvi``,
    ``optimize``, ``FASO``, ``RAABBVI`` and the device-resident fit.  Everything that needs one fixed density raises
    ``NotImplementedError`` and points to :meth:`full_model`: ``DISInclusiveKL`` and ``AlphaDivergence`` (a subsampled log
    density inside an importance weight is biased), the RGE control variates, ``_hessian_vector_product``, ``hmc``,
    ``find_mode``, ``hessian``, ``laplace_approximation``, ``vi_diagnostics``, ``loo``, ``predict``,
    ``samples_and_log_weights`` and a sharded engine.  Not in the reference."""

    _LINKS = _GLM_LINKS
    _ORDERS = {'sequential': 0, 'shuffle': 1}
    FEISTEL_ROUNDS = 6

    def __init__(self, X, y, batch_size, likelihood='logistic', prior_sd=10.0, noise_sd=1.0, seed=0, order='shuffle'):
        X = np.ascontiguousarray(X, dtype=np.float64)
        y = np.asarray(y, dtype=np.float64)
        if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1 or y.shape != (X.shape[0],):
            raise ValueError('X must be (n_data, p) with n_data, p >= 1 and y (n_data,)')
        if X.shape[0] >= 1 << 31:
            raise ValueError('n_data must be below 2^31')
        if isinstance(batch_size, (bool, np.bool_)) or not isinstance(batch_size, (int, np.integer)) \
                or not 1 <= int(batch_size) <= X.shape[0]:
            raise ValueError('batch_size must be an integer in [1, n_data = {}]; got {!r}'.format(X.shape[0], batch_size))
        if likelihood not in self._LINKS:
            raise ValueError("likelihood must be 'logistic', 'poisson' or 'gaussian'")
        if order not in self._ORDERS:
            raise ValueError("order must be 'shuffle' or 'sequential'")
        if not prior_sd > 0 or not noise_sd > 0:
            raise ValueError('prior_sd and noise_sd must be positive')
        if isinstance(seed, (bool, np.bool_)) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 1 << 64:
            raise ValueError('seed must be an integer in [0, 2^64)')
        _check_glm_response(likelihood, y)
        self.X, self.y, self.likelihood, self.order = X, y, likelihood, order
        self.prior_sd, self.noise_sd, self.seed = float(prior_sd), float(noise_sd), int(seed)
        self._batch_size = int(batch_size)
        self._batch_box = [0]        # shared with the engine binding through device_spec (Engine.set_model pushes it)
        super().__init__(X.shape[1])

    def _build_spec(self):
        seed = self.seed - (1 << 64) if self.seed >= 1 << 63 else self.seed      # the 64 bits as an int64
        return (_lib.MODEL_MINIBATCH_GLM, self._dim,
                np.concatenate([self.X.ravel(), self.y, [self.prior_sd, self.noise_sd]]),
                np.array([self.X.shape[0], self._batch_size, self._LINKS[self.likelihood], self._ORDERS[self.order], seed],
                         dtype=np.int64),
                self._batch_box)

    @property
    def n_data(self):
        return self.X.shape[0]

    @property
    def batch_size(self):
        return self._batch_size

    @property
    def batch(self):
        """Number of the batch the next evaluation uses (settable; setting it back replays the same batches)."""
        return self._batch_box[0]

    @batch.setter
    def batch(self, t):
        if isinstance(t, (bool, np.bool_)) or not isinstance(t, (int, np.integer)) \
                or not 0 <= int(t) < (1 << 62) // self._batch_size - 1:
            raise ValueError('batch must be an integer in [0, 2^62 / batch_size - 1); got {!r}'.format(t))
        self._batch_box[0] = int(t)

    @property
    def epoch(self):
        """Epoch of the first position of batch ``self.batch``: ``batch * batch_size // n_data``."""
        return self.batch * self._batch_size // self.n_data

    def batch_indices(self, t=None):
        """The observations of batch ``t`` (None: ``self.batch``) in batch order, int64 ``(batch_size,)``: the host
        restatement of the engine's index kernel (``vb_minibatch_indices`` gives the device's)."""
        t = self.batch if t is None else t
        if isinstance(t, (bool, np.bool_)) or not isinstance(t, (int, np.integer)) \
                or not 0 <= int(t) < (1 << 62) // self._batch_size - 1:
            raise ValueError('t must be an integer in [0, 2^62 / batch_size - 1); got {!r}'.format(t))
        n, B = self.n_data, self._batch_size
        q = np.uint64(int(t) * B) + np.arange(B, dtype=np.uint64)
        slots, epochs = q % np.uint64(n), q // np.uint64(n)
        if self.order == 'sequential':
            return slots.astype(np.int64)
        w = max(1, ((n - 1).bit_length() + 1) // 2)
        ws, mask = np.uint64(w), np.uint64((1 << w) - 1)
        k0, k1 = self.seed & 0xFFFFFFFF, self.seed >> 32
        x = slots.copy()
        todo = np.arange(B)
        while todo.size:           # cycle walk: the elements whose image is not below n_data yet
            e = epochs[todo]
            left, right = x[todo] >> ws, x[todo] & mask
            for r in range(self.FEISTEL_ROUNDS):
                f = _philox4x32_10_word0(right, np.uint64(r), e & _M32, e >> _S32, k0, k1) & mask
                left, right = right, left ^ f
            x[todo] = (left << ws) | right
            todo = todo[x[todo] >= np.uint64(n)]
        return x.astype(np.int64)

    def full_model(self):
        """The same data as a full-batch target: the :class:`LogisticRegressionModel`, :class:`PoissonRegressionModel`
        or :class:`LinearRegressionModel` on this model's ``X`` (not copied) and ``y``."""
        if self.likelihood == 'logistic':
            return LogisticRegressionModel(self.X, self.y, self.prior_sd)
        if self.likelihood == 'poisson':
            return PoissonRegressionModel(self.X, self.y, self.prior_sd)
        return LinearRegressionModel(self.X, self.y, self.prior_sd, self.noise_sd)

    def pointwise_log_likelihood(self, x):
        """``log p(y_j | x_j' theta_s)`` of the observations ``j`` of batch ``self.batch``, in batch order, for every draw
        (row of ``x``): ``(S, batch_size)``.  Normalised densities, NOT scaled by ``n_data / batch_size``, without the
        prior (``vb_minibatch_pointwise``).  ``x``: (S, D), or (D,) for one draw."""
        x, _ = self._rows(x)
        eng = _lib.default_engine()
        eng.set_model(self.device_spec())
        return eng.minibatch_pointwise(x, self._batch_size)

    def hessian(self, x):
        refuse_minibatch(self, 'hessian()')

    def _refuse_ksd(self):
        refuse_minibatch(self, 'ksd_from_draws()')

    def _refuse_svgd(self, what):
        refuse_minibatch(self, what)

    def _value_grad_hessian(self, x, want_hessian=True):
        refuse_minibatch(self, 'find_mode() / laplace_approximation()')

    def find_mode(self, x0=None, max_iter=100, tol=1e-10):
        refuse_minibatch(self, 'find_mode()')
