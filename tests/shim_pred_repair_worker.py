"""tests/shim_operator_worker.py for a cloud its case dictionary cannot express (TEST INFRASTRUCTURE): the noisy
lidar-like reflectance slice of tests/pred_repair_cases.py with three direct predictors -- the content whose mode
decisions the device's whole-slice passes do not settle.  The worker's own main() runs; only the function that
makes a predicting case is replaced.

    python tests/shim_pred_repair_worker.py <case json>     (transform 1, "n", "qp", "lib")"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import shim_operator_worker as w  # noqa: E402


def pred_case(case):
    import pred_repair_cases as pc
    xyz, attrs, lp = pc.lidar(case["n"])
    return xyz, attrs, lp, pc.params([len(xyz)], lp, case["qp"]), 4, case["qp"]


if __name__ == "__main__":
    w.pred_case = pred_case
    w.main()
