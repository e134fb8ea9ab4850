"""Child process of test_gpu_spmk_limits.test_epoch_wrap: the one-launch powers step with its flag epoch about to cross 2^31 and
2^32.  Runs on libmi355spmv_dev.so (MI355_SPMV_LIBRARY, read once per process) with MI355_SPMK_FUSED=1.  Per case and epoch e: a
k = 2 step sets the handle's step up, mi_debug_spmk_set_epoch(A, e) leaves every run's flag at e - 1 and the next launch counting
from e, then k = 4 three times with a fresh x each (flags e + 1 .. e + 3, e + 5 .. e + 7, e + 9 .. e + 11 — through the sign bit, or
through zero), every power bitwise against the chained oracle; the call after them must not report a give-up."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import spmk_cases as C  # noqa: E402
from navierstokes_amd import mpk  # noqa: E402
from oracle import oracle as O  # noqa: E402


def main():
    L = mpk.lib()
    assert hasattr(L, "mi_debug_spmk_set_epoch"), "not the devtools build"
    assert os.environ.get("MI355_SPMK_FUSED") == "1"
    rng = np.random.default_rng(31)
    for name in ("band:2000:7", "s15:66000:300"):
        n, p, c, v = C.build(name)
        A = mpk.csrmatrix(n, p, c, v).set_kernel("ring")
        outs = [torch.empty(n, dtype=torch.float64, device="cuda") for _ in range(4)]

        def step(k, what):
            x = rng.uniform(-1.0, 1.0, n)
            for t in outs:
                t.fill_(float("nan"))
            mpk.SpMkV(outs[:k], torch.from_numpy(x).cuda(), A)  # raises if an earlier step's wait gave up
            torch.cuda.synchronize()
            assert A.spmk_info(k)["one_launch"], (name, what, A.spmk_info(k))
            Y = O.spmk_chain(k, p, c, v, x)
            for q in range(k):
                bad = np.nonzero(outs[q].cpu().numpy().view(np.uint64) != Y[q].view(np.uint64))[0]
                assert bad.size == 0, f"{name} {what}, power {q + 1}: {bad.size} entries differ, first at {bad[:5]}"

        step(2, "set-up")
        for e in (2**31 - 3, 2**32 - 3):
            mpk.check(L.mi_debug_spmk_set_epoch(A.handle, e))
            for rep in range(3):
                step(4, f"epoch {e} + {4 * rep}")
            step(2, f"the call after epoch {e}")
            print(f"epoch {e}: {name} ok", flush=True)
        A.close()
    print("SPMK_EPOCH_OK")


if __name__ == "__main__":
    main()
