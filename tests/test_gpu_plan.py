"""GPU: the plan a live context holds is the plan ka_debug_plan makes on the host for the device's CU count -- after an upload,
after a switch flipped with reload_env, after a subset planned with tree_plan_tasks.  Upload only: no kernel runs."""
import sys

import numpy as np
import pytest

from util import GOLDEN

sys.path.insert(0, GOLDEN)
import make_golden_plan as mp  # noqa: E402


def same(x, y):
    from kalign_amd import api
    return all(x[k] == y[k] for k in api.PLAN_SCALARS) and all(np.array_equal(x[a], y[a]) for a in mp.ARRAYS)


@pytest.mark.gpu
def test_context_holds_the_plan_the_host_makes(monkeypatch):
    """case a (40 sequences: no queued launch) and case c (2560: about the smallest bisecting tree whose first mixed level holds
    more tasks than 256 CUs, which a queued launch needs)"""
    import bench
    import torch
    import kalign_amd
    from kalign_amd import api
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    for k in mp.PLAN_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    subm, scal = bench.scoring(False)
    ctx = kalign_amd.Context(0)
    try:
        for name in ("a", "c"):
            job = mp.case_inputs(name)
            lens, tasks = job["lens"], job["tasks"]
            codes = [np.zeros(n, np.uint8) for n in lens]
            monkeypatch.delenv("KA_NO_QUEUE", raising=False)
            ctx.reload_env()
            ctx.tree_upload(codes, tasks, subm, scal, None)
            default = ctx.debug_plan(n_cus)
            assert same(default, api.debug_plan(lens, tasks, n_cus)), name
            monkeypatch.setenv("KA_NO_QUEUE", "1")
            ctx.reload_env()
            flipped = ctx.debug_plan(n_cus)
            assert same(flipped, api.debug_plan(lens, tasks, n_cus)), name
            if name == "c":                                  # (the switch takes the queued launch out of the plan)
                assert default["queue_first"] >= 0 and flipped["queue_first"] == -1
            ids = mp.case_inputs("i")["task_ids"] if name == "c" else np.flatnonzero(tasks[:, 2] < tasks[len(tasks) // 2, 2])
            ctx.tree_plan_tasks(ids)
            assert same(ctx.debug_plan(n_cus), api.debug_plan(lens, tasks, n_cus, task_ids=ids)), name
    finally:
        ctx.close()
