"""The planner's own cost on the host: ka_debug_plan (task preparation + plan_launches, no GPU) on a 16384-sequence bisecting
tree for a device of 256 CUs, default switches -- the median of 20 calls, as one JSON line (profiles/plan_time.jsonl keeps them).

    python tools/plan_time.py [LABEL]
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kalign_amd import api, guide  # noqa: E402

N, N_CUS, CALLS = 16384, 256, 20
tasks = guide.bisecting_tree(N, seed=1)
lens = np.random.RandomState(1).randint(340, 461, N).astype(np.int32)
for k in [k for k in os.environ if k.startswith("KA_")]:
    del os.environ[k]
api.debug_plan(lens, tasks, N_CUS)
ms = []
for _ in range(CALLS):
    t0 = time.perf_counter()
    api.debug_plan(lens, tasks, N_CUS)
    ms.append(1e3 * (time.perf_counter() - t0))
print(json.dumps(dict(label=sys.argv[1] if len(sys.argv) > 1 else "", sequences=N, n_cus=N_CUS, calls=CALLS,
                      median_ms=round(float(np.median(ms)), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3))))
