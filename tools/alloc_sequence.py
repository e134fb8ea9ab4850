#!/usr/bin/env python3
"""The sequence of device allocations and frees of one life of every kind of CSR / BCSR handle (profiles/NOTES.md R9.1), or of
every kind of partition and mi_dist handle (R10.1): where a handle's allocations and frees land moves launch times (§4.12), so a
change to how handles own their memory is held to the sequence its parent made.

  rocprofv3 --hip-trace --output-format csv -d OUT -o life -- python tools/alloc_sequence.py life
  python tools/alloc_sequence.py reduce OUT > sequence.txt      (one line per hipMalloc / hipHostMalloc / hipFree / hipHostFree call)
  python tools/alloc_sequence.py reduce OUT threads > sequence.txt   (the same per thread: the first thread's calls, then every other
                                                                      thread's as one block, the blocks sorted by content — an mi_dist
                                                                      handle's ranks are worker threads, whose calls interleave by chance)

`part` in place of `life` runs one cycle of tests/test_gpu_part_lifecycle.py (tests/multirank_worker.lifecycle_cycle); the caller sets
what that test's child gets: MI355_SPMV_LIBRARY (a devtools build: the parent's or this tree's), MI355_PUSH_LOOPBACK=1 and
MI355_RCCL_LIBRARY=tests/fake_rccl/libfake_rccl.so.

`life` runs tests/test_gpu_csr_lifecycle.all_lives once, in a fresh process, and prints what the create-time measurements chose
(a sliced copy that loses its race is released: two runs agree only where the choices do); ALLOC_SEQUENCE_PACKAGE_ROOT=<tree> takes
the navierstokes_amd package, and with it the library, of another checkout (the parent's build), the test and the oracle of this one.  `reduce` reads the trace's
hip_api_trace CSV; where it carries no arguments, the sequence is the order of the calls alone."""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("hipMalloc", "hipHostMalloc", "hipExtMallocWithFlags", "hipMallocAsync", "hipFree", "hipHostFree", "hipFreeAsync",
         "hipStreamCreate", "hipStreamCreateWithFlags", "hipStreamDestroy", "hipEventCreate", "hipEventCreateWithFlags", "hipEventDestroy",
         "hipIpcOpenMemHandle", "hipIpcCloseMemHandle")


def life():
    sys.path[:0] = [os.environ.get("ALLOC_SEQUENCE_PACKAGE_ROOT", ROOT), os.path.join(ROOT, "tests"), ROOT]
    import torch
    import test_gpu_csr_lifecycle as T
    from navierstokes_amd import mpk
    (p, c, v), scrambled = T.matrices()
    R, Rs = T.reference(p, c, v, 1), T.reference(*scrambled, 2)
    torch.cuda.synchronize()
    print("library:", mpk.lib()._name)
    for name, (pp, cc, vv), e in (("natural", (p, c, v), {}), ("relabelled", scrambled, {"MI355_REORDER": "1"})):
        with T.env(**e):
            A = mpk.csrmatrix(len(pp) - 1, pp, cc, vv)
            print(f"choices, {name}: kernel {A.kernel_name()}, sliced copy kept {A.sstream_info()['built']}, tile {A.tile_info()['built']}, "
                  f"mring {A.mring_info()['built']}")
            A.close()
    torch.cuda.synchronize()
    print("BEGIN LIVES", flush=True)
    T.all_lives(R, Rs, T.side_streams(), "traced")
    torch.cuda.synchronize()
    print("END LIVES", flush=True)


def part():
    sys.path[:0] = [os.path.join(ROOT, "tests"), ROOT]
    import torch
    import multirank_worker as W
    from navierstokes_amd import mpk
    torch.cuda.set_device(0)
    ref = W.lifecycle_reference()
    torch.cuda.synchronize()
    print("library:", mpk.lib()._name)
    print("BEGIN LIVES", flush=True)
    W.lifecycle_cycle(ref, 0, print)  # (two runs agree only where the pieces' create-time choices do)
    torch.cuda.synchronize()
    print("END LIVES", flush=True)


def reduce(out_dir, by_thread=False):
    files = sorted(glob.glob(os.path.join(out_dir, "**", "*hip_api_trace.csv"), recursive=True))
    if not files:
        sys.exit(f"no hip_api_trace.csv under {out_dir}")
    rows = []
    for f in files:
        with open(f, newline="") as fh:
            rows += list(csv.DictReader(fh))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    with_args = [k for k in rows[0] if k.lower() in ("args", "arguments")]
    print(f"# {len(rows)} HIP calls; arguments in the trace: {'yes' if with_args else 'no (order of calls only)'}")
    if not by_thread:
        for r in rows:
            if r["Function"] in CALLS:
                print(r["Function"], r[with_args[0]] if with_args else "")
        return
    tid = [k for k in rows[0] if k.lower() in ("thread_id", "tid")][0]
    threads = {}
    for r in rows:
        if r["Function"] in CALLS:
            threads.setdefault(r[tid], []).append(r["Function"])
    first = rows[0][tid]
    blocks = [threads.pop(first, [])] + sorted(threads.values())
    for i, b in enumerate(blocks):
        print(f"# thread {i}: {len(b)} calls")
        print("\n".join(b))


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "life":
        life()
    elif len(sys.argv) == 2 and sys.argv[1] == "part":
        part()
    elif len(sys.argv) in (3, 4) and sys.argv[1] == "reduce":
        reduce(sys.argv[2], by_thread=sys.argv[3:] == ["threads"])
    else:
        sys.exit(__doc__)
