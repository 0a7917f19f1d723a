"""Host cost of one call through the ctypes binding (bonai_amd.lib), no device involved: loft_conv_wgrad_form (20 arguments:
15 int, 5 host int arrays) and loft_nms_workspace_bytes (3 int64).  Both are host-only queries, so the time is argument
conversion + the foreign call.  Scalars are plain Python ints as at the call sites of bonai_amd.kernels; the arrays are built
once.  Prints every repeat (ns per call) and the median, for same-machine A/B of two checkouts.
usage: python abi_call_time.py [calls per repeat] [repeats]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: F401  (load torch's HIP runtime before libloft_hip.so)
from bonai_amd import lib as L


def repeats(fn, args, calls, reps):
    out = []
    for _ in range(reps + 1):                # the first repeat warms up and is dropped
        t = time.perf_counter_ns()
        for _ in range(calls):
            fn(*args)
        out.append((time.perf_counter_ns() - t) / calls)
    return sorted(out[1:])


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 9
    lib = L.load()
    taps = [(0, 0, dy, dx, 3 * (dy + 1) + dx + 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]     # a 3x3, pad 1, on a 64 x 64 map
    A = [L.arr(L.c_int, [t[i] for t in taps]) for i in range(5)]
    cases = (('loft_conv_wgrad_form', (2, 64, 64, 256, 64, 64, 256, 64, 64, 1, 1, len(taps), *A, 1, 0, 0)),
             ('loft_nms_workspace_bytes', (120000, 3000, 40)))
    for name, args in cases:
        fn = getattr(lib, name)
        r = repeats(fn, args, calls, reps)
        print(f'{name:26s} {len(args):2d} args  result {fn(*args):6d}  median {r[len(r) // 2]:7.1f} ns/call  '
              f'min {r[0]:7.1f}  max {r[-1]:7.1f}  repeats ' + ' '.join(f'{x:.1f}' for x in r))


if __name__ == '__main__':
    main()
