"""One recorder for the tests that hold a step bit-equal to a recording made on the MI355X with the parent commit's library
(tests/golden/*_step_parent.npz: test_gpu_stereo.py, test_gpu_sam3d.py, test_gpu_smart_pose.py)."""
import numpy as np


def record_step(lib, problem, values, jac_types, pcg=True):
    """Everything the error, one linearisation, two damped lambda tries and (pcg) one PCG try of `problem` at `values` compute, by the
    names the recordings use; jac_types: the factor types whose records are kept as jac<type>."""
    dev = lib.DeviceGraph(problem)
    dev.set_values(values)
    got = {"error": np.float64(dev.error())}
    dev.linearize()
    for ft in jac_types:
        got[f"jac{ft}"] = dev.jacobians(ft)
    got["hessian_diagonal"], got["gradient"] = dev.hessian_diagonal(), dev.gradient()
    for i, (lam, dd) in enumerate(((1e-3, False), (1e-4, True))):
        rc, out = dev.try_lambda(lam, dd)
        got[f"rc{i}"], got[f"out{i}"], got[f"delta{i}"], got[f"trial{i}"] = np.int64(rc), out, dev.delta(), dev.trial_values()
    if pcg:
        rc, out, its = dev.try_lambda_pcg(1e-3, False, max_iterations=300, min_iterations=1, epsilon_rel=1e-10, epsilon_abs=1e-14)
        got["rc_pcg"], got["out_pcg"], got["delta_pcg"], got["its_pcg"] = np.int64(rc), out, dev.delta(), np.int64(its)
    dev.close()
    return got
