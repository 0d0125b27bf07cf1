"""bench.py --dump-outputs on the GPU: the arrays it writes are what the timed path computed -- the assembled rhs and the Newton
update of a one-context InsIM run of the same channel, entry for entry at the dumped global dof ids."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_dumped_outputs_are_the_timed_step(tmp_path):
    d = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--cells", "16", "--steps", "2", "--warmup", "1",
           "--cpu-cells", "0", "--fgmres-rel", "1e-9", "--inner-rel", "1e-4", "--inner-rel-first", "0", "--extras", "0",
           "--tuned", "0", "--fsi", "0", "--cylinder-legs", "0", "--dump-outputs", str(d)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=tmp_path)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    got = {k: np.load(d / f"{k}.npy") for k in ("update", "rhs", "dof_index", "solve_stats")}
    assert all(a.dtype == np.float64 for a in got.values())
    sys.path.insert(0, ROOT)
    from openifem_amd import capi, host
    S = host.InsIM(host.channel_prm(3), (16, 16, 16), (0, 0, 0), (2.0, 0.2, 0.2))
    S.setup(0)
    S.opts.inner_rel, S.opts.inner_rel_first, S.opts.fgmres_rel = 1e-4, 0.0, 1e-9
    S.channel_state()
    for _ in range(3):
        S.assemble(False)
        st = S.solve(False)
    _, n_u, n_p = S.sizes()
    t = S.partition_tables()
    np.testing.assert_array_equal(got["dof_index"], np.arange(n_u + n_p))  # below the sample size: every dof
    ref = {}
    for name, vec in (("update", capi.VEC_UPDATE), ("rhs", capi.VEC_RHS)):
        x = np.zeros(n_u + n_p)
        assert S.L.ifem_vec_get(S.ctx, vec, x.ctypes.data_as(C.c_void_p)) == 0
        g = np.full(n_u + n_p, np.nan)
        g[(t["l2g_u"][:, None] * 3 + np.arange(3)[None, :]).ravel()] = x[:n_u]
        g[3 * t["n_unodes_global"] + t["l2g_p"]] = x[n_u:]
        ref[name] = g
    S.close()
    assert not np.isnan(ref["update"]).any() and np.linalg.norm(ref["update"]) > 0
    assert np.abs(got["rhs"] - ref["rhs"]).max() <= 1e-11 * np.abs(ref["rhs"]).max()
    assert np.linalg.norm(got["update"] - ref["update"]) <= 1e-6 * np.linalg.norm(ref["update"])
    assert abs(got["solve_stats"][0] - st.fgmres_iters) <= 1
    # the absolute residual of the last outer solve, against its stopping rule max(fgmres_abs 1e-12, fgmres_rel ||b||)
    assert 0 < got["solve_stats"][1] <= 1.05 * max(1e-12, 1e-9 * np.linalg.norm(ref["rhs"]))
