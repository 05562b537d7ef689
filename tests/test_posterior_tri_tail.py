"""The posterior's Lw steps leave out the products with the zero half of Lw's diagonal blocks (GPCORE_POSTERIOR_TRI, default on; 0 = the
full product).  The skipped matrix instructions would add +-0 * a to an accumulator, so for finite inputs the two settings must agree
BIT FOR BIT: every comparison between them is np.array_equal.  Both settings also meet the oracle at the tolerances of
tests/test_gpu_parity.py::test_predict_many_points_small_model (mean 1e-9 of max(1, max|mean|), variance 1e-9 sf^2).

GPCORE_ROWS_LEFT_MIN=1 puts every batch on the Lw path.  The 256-row kernel takes a launch only when it has more than 64 row tiles of
256 (fewer fill more CUs as 128-row tiles), hence m = 16 768 = 65 tiles of 256 rows + one of 128: both kernels run in every step.
Entry points are the device-pointer ones the benchmark uses (gp_fit_rbf_dev, gp_predict_dev, gp_model_append_dev)."""
import ctypes as C
import os

import numpy as np
import pytest

from gp_algos_amd import _lib as L
from gp_algos_amd import synth
from oracle import gp_oracle as orc

pytestmark = pytest.mark.gpu

TOL_MEAN = 1e-9       # tests/test_gpu_parity.py
TOL_VAR = 1e-9
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "posterior_full_product_n384_m16768.npy")


@pytest.fixture(scope="module")
def ctx():
    from gp_algos_amd.core import Context
    c = Context(0)
    yield c
    c.close()


_PROBLEMS, _ORACLE = {}, {}


def _problem(n, m, seed):
    if (n, m, seed) not in _PROBLEMS:
        _PROBLEMS[(n, m, seed)] = synth.regression(n, 3, m, seed, seed + 1, seed + 2, synth.ard_theta(3, 1.2, 1.0, 0.15))
    return _PROBLEMS[(n, m, seed)]


def _oracle(n, m, seed):
    """(mean, var) of the oracle, computed once per problem and shared."""
    if (n, m, seed) not in _ORACLE:
        p = _problem(n, m, seed)
        Lo, ao = orc.fit(p["X"], p["y"], p["theta"])
        om, ov, _, _ = orc.predict(p["X"], p["theta"], Lo, ao, p["Xs"])
        _ORACLE[(n, m, seed)] = (om, ov)
    return _ORACLE[(n, m, seed)]


class _DevModel:
    """gp_fit_rbf_dev on the first n0 training points; predict() is gp_predict_dev at all test points under one setting of the switch."""

    def __init__(self, ctx, p, n0=None):
        self.ctx, self.p, self.lib = ctx, p, ctx._lib
        n, d = p["X"].shape
        self.n0 = n if n0 is None else n0
        self.m = p["Xs"].shape[0]
        self.dX, self.dy, self.dXs = ctx.upload(p["X"][:self.n0]), ctx.upload(p["y"][:self.n0]), ctx.upload(p["Xs"])
        self.dmean, self.dvar = ctx.dev_alloc(8 * self.m), ctx.dev_alloc(8 * self.m)
        self.extra = []
        self.h, info = C.c_void_p(), C.c_int()
        theta = L.f64(p["theta"])
        ctx.check(self.lib.gp_fit_rbf_dev(ctx.h, self.dX, self.n0, d, self.n0, self.dy, L.dptr(theta), float("nan"), C.byref(self.h), C.byref(info)),
                  info.value)

    def append_rest(self):
        p, n0 = self.p, self.n0
        k = p["X"].shape[0] - n0
        dXn, dyn = self.ctx.upload(p["X"][n0:]), self.ctx.upload(p["y"][n0:])
        self.extra += [dXn, dyn]
        info = C.c_int()
        self.ctx.check(self.lib.gp_model_append_dev(self.h, dXn, k, k, dyn, C.byref(info)), info.value)

    def predict(self, monkeypatch, tri):
        if tri is None:
            monkeypatch.delenv("GPCORE_POSTERIOR_TRI", raising=False)      # the default: on
        else:
            monkeypatch.setenv("GPCORE_POSTERIOR_TRI", tri)
        self.ctx.check(self.lib.gp_predict_dev(self.h, self.dXs, self.m, self.m, self.dmean, self.dvar))
        return self.ctx.download(self.dmean, (self.m,)), self.ctx.download(self.dvar, (self.m,))

    def close(self):
        self.lib.gp_model_destroy(self.h)
        for q in [self.dX, self.dy, self.dXs, self.dmean, self.dvar] + self.extra:
            self.ctx.dev_free(q)


def _meets_oracle(mean, var, ref, sf2, label):
    om, ov = ref
    em, ev = np.max(np.abs(mean - om)), np.max(np.abs(var - ov))
    print("%s: max|dmean| %.3e  max|dvar| %.3e" % (label, em, ev))
    assert em <= TOL_MEAN * max(1.0, np.max(np.abs(om))), label
    assert ev <= TOL_VAR * sf2, label


# n = 384: three block columns -- the first step is all tail, then a middle and a last step.  n = 200: padded to 256 with an identity
# pad block, m = 16 700 leaves pad rows in the last tile.  n = 256, m = 384: three 128-row tiles, every launch on the 128-row kernel.
@pytest.mark.parametrize("n,m,seed", [(384, 16768, 201), (200, 16700, 211), (256, 384, 221)],
                         ids=["both-kernels-n384", "padded-n200", "128-row-kernel-only"])
def test_bit_identity_and_oracle_parity(ctx, monkeypatch, n, m, seed):
    monkeypatch.setenv("GPCORE_ROWS_LEFT_MIN", "1")
    p = _problem(n, m, seed)
    mdl = _DevModel(ctx, p)
    full = mdl.predict(monkeypatch, "0")
    tri = mdl.predict(monkeypatch, None)
    again = mdl.predict(monkeypatch, "0")
    mdl.close()
    assert np.all(np.isfinite(full[0])) and np.all(np.isfinite(full[1]))
    assert np.array_equal(full[0], again[0]) and np.array_equal(full[1], again[1])      # the comparison below is between settings, not runs
    assert np.array_equal(tri[0], full[0]), "mean differs in %d places" % np.count_nonzero(tri[0] != full[0])
    assert np.array_equal(tri[1], full[1]), "variance differs in %d places" % np.count_nonzero(tri[1] != full[1])
    sf2 = p["theta"][0] ** 2
    _meets_oracle(full[0], full[1], _oracle(n, m, seed), sf2, "full product")
    _meets_oracle(tri[0], tri[1], _oracle(n, m, seed), sf2, "triangular tail")


def test_bit_identity_after_an_append(ctx, monkeypatch):
    """Lw is valid when 128 points are appended to n = 256: the model grows by a block (Lw's new block row is [0 | I]) and the block row
    is rebuilt by the single-block form of build_lw.  The result is also the oracle's fit on all 384 points, at the tolerances of
    tests/test_gpu_model_append.py (mean 1e-9 of max(1, |mean|), variance 1e-9 sf^2)."""
    monkeypatch.setenv("GPCORE_ROWS_LEFT_MIN", "1")
    n, m, seed = 384, 16768, 201
    p = _problem(n, m, seed)
    mdl = _DevModel(ctx, p, n0=256)
    mdl.predict(monkeypatch, None)          # builds Lw
    mdl.append_rest()
    full = mdl.predict(monkeypatch, "0")
    tri = mdl.predict(monkeypatch, None)
    mdl.close()
    assert np.array_equal(tri[0], full[0]) and np.array_equal(tri[1], full[1])
    om, ov = _oracle(n, m, seed)
    assert np.max(np.abs(tri[0] - om) / np.maximum(1.0, np.abs(om))) <= 1e-9
    assert np.max(np.abs(tri[1] - ov)) <= 1e-9 * p["theta"][0] ** 2


def test_full_product_kernels_give_the_recorded_bits(ctx, monkeypatch):
    """The general instantiations of the two row-tile kernels (GPCORE_POSTERIOR_TRI=0; they are what every other caller runs) against
    the output of the build before the tail variant existed, recorded on an MI355X at this seed: [mean; var], bit for bit."""
    monkeypatch.setenv("GPCORE_ROWS_LEFT_MIN", "1")
    p = _problem(384, 16768, 201)
    mdl = _DevModel(ctx, p)
    mean, var = mdl.predict(monkeypatch, "0")
    mdl.close()
    gold = np.load(GOLDEN)
    assert gold.shape == (2, 16768)
    assert np.array_equal(mean, gold[0]) and np.array_equal(var, gold[1])
