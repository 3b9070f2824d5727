"""jacobian_nemesis with ISCAT = 3 (SINGLE_SCATTERING_PLANE_PARALLEL) through the drop-in subclass: the reference forces the
numerical route (ForwardModel_0.py:2251-2252), the staged route runs the reference's host code per state and sends the NX + 1
states to the engine's batched single-scattering entry in ONE call per (geometry, averaging point).  The engine is a double
answered by the CPU oracle; the case is the one tests/golden/jacobian_ss.npz was recorded on
(tools/golden/gen_golden_jacobian_ss.py)."""
import importlib.util
import os
import shutil
import sys
import tempfile

import numpy as np
import pytest

import singlescatt_cases as sc
from test_dropin_reference import OracleEngineDouble

REF = "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = [pytest.mark.needs_reference,
              pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "archnemesis")), reason="reference tree not present")]


class BatchingDouble(OracleEngineDouble):
    """... with ansfm_cirsrad_ck_singlescatt_batch answered model by model by the single-model answer; counts both kinds of call"""
    def __init__(self, orc):
        super().__init__(orc)
        self.ss_batches, self.ss_alone, self._in_batch = [], 0, False

    def cirsrad_ck_singlescatt(self, *a, **k):
        if not self._in_batch:
            self.ss_alone += 1
        return super().cirsrad_ck_singlescatt(*a, **k)

    def cirsrad_ck_singlescatt_batch(self, ISPACE, lp, lt, am, taucont, tausca, phase, NLAYIN, LAYINC, SCALE, EMTEMP, TSURF, EMIS, BRDF,
                                     SOLF, sol, emi, xfac=None):
        n = np.shape(lp)[0]
        assert np.shape(phase)[0] == n and np.shape(SCALE)[0] == n and np.shape(TSURF) == (n,)
        self.ss_batches.append(n)
        self._in_batch = True
        try:
            return np.stack([self.cirsrad_ck_singlescatt(ISPACE, lp[m], lt[m], am[m], taucont[m], tausca[m], phase[m], NLAYIN, LAYINC,
                                                         SCALE[m], EMTEMP[m], float(TSURF[m]), EMIS, BRDF, SOLF, sol, emi, xfac=xfac)
                             for m in range(n)])
        finally:
            self._in_batch = False

    def last_layer_rows(self):
        return 0, 0


def _generator():
    spec = importlib.util.spec_from_file_location("gen_golden_jacobian_ss", os.path.join(ROOT, "tools", "golden", "gen_golden_jacobian_ss.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture()
def ss_case(oracle, monkeypatch):
    """The cut ISCAT = 3 case in a scratch directory, the reference imported; run(double, route) -> YN, KK, info"""
    from oracle.ref_import import import_reference
    from oracle import gen_golden_jacobian as gj
    import archnemesis_dist_amd.forward_model as fmod
    gs = _generator()
    ans = import_reference()
    work = tempfile.mkdtemp(prefix="ansfm_jacss_drop_")
    gj.setup_c1(ans, work, seed=4, case=gs.CASE)
    cwd = os.getcwd()
    os.chdir(work)
    fmod.set_strict(True)
    fmod.reset_summary()

    def run(double, route):
        monkeypatch.setattr(fmod, "get_engine", lambda device=0: double)
        fm = gs.cut_case(ans, cls=fmod.make_gpu_forward_model(ans.ForwardModel_0))
        fm.ansfm_jacobian_route = route
        XN0 = np.array(fm.Variables.XN)
        YN, KK = fm.jacobian_nemesis(NCores=1, analytical_gradient=True)          # ISCAT = 3: numerical whatever is asked
        assert np.array_equal(fm.Variables.XN, XN0)
        info = fm.ansfm_last_jacobian
        assert info["nfm"] == 9 and info["analytic_columns"] == 0
        return YN, KK, info
    try:
        yield run
    finally:
        fmod.set_strict(False)
        os.chdir(cwd)
        shutil.rmtree(work, ignore_errors=True)


def _against_fixture(YN, KK, golden_dir):
    z = np.load(os.path.join(golden_dir, "jacobian_ss.npz"))
    np.testing.assert_allclose(YN, z["YN"], rtol=2e-7)
    sc.assert_kk(KK, z, 1e-4)


def test_staged_route_sends_the_states_to_the_batched_entry_in_one_call(ss_case, oracle, golden_dir):
    """`auto` cannot take the profile route (scattering, an aerosol model) and lands on the staged one: exactly one batched call for
    the nine states of the one (geometry, averaging point), no state on its own; YN and KK equal the loop route's (the reference's
    execute_fm per column on the same objects) and the reference's own (fixture)."""
    double = BatchingDouble(oracle)
    YN, KK, info = ss_case(double, "auto")
    assert info["route"] == "staged"
    assert double.ss_batches == [9] and double.ss_alone == 0
    _against_fixture(YN, KK, golden_dir)
    loop = BatchingDouble(oracle)
    YN_l, KK_l, info_l = ss_case(loop, "loop")
    assert info_l["route"] == "loop" and loop.ss_batches == [] and loop.ss_alone == 9
    assert np.array_equal(YN, YN_l) and np.array_equal(KK, KK_l)


def test_an_engine_without_the_batched_entry_runs_the_states_alone(ss_case, oracle, golden_dir):
    """An engine object that lacks cirsrad_ck_singlescatt_batch: the staged route runs every state through CIRSrad on its own, as
    before, and agrees."""
    double = OracleEngineDouble(oracle)
    assert not hasattr(double, "cirsrad_ck_singlescatt_batch")
    YN, KK, info = ss_case(double, "staged")
    assert info["route"] == "staged" and double.ss_calls == 9
    _against_fixture(YN, KK, golden_dir)
    batched = BatchingDouble(oracle)
    YN_b, KK_b, _ = ss_case(batched, "staged")
    assert batched.ss_batches == [9] and np.array_equal(YN, YN_b) and np.array_equal(KK, KK_b)
