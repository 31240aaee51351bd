"""Writes tests/golden/tails_k2.npz and tests/golden/tails_k3.npz: the inputs and mpmath expectations the device p-value
tails (K2) and the window combine (K3) are pinned to (tests/tail_ref.py holds the definitions; tests/test_tails.py checks
that a new run reproduces the committed files bit for bit; tests/test_tails_gpu.py needs numpy only).

    python oracle/gen_tail_golden.py

Deterministic: fixed seeds, numpy's PCG64 uniforms, plain additions, and mpmath (pure Python) for every transcendental.
Needs mpmath; reads nothing but tests/tail_ref.py."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))
import tail_ref as T  # noqa: E402


def main():
    k2 = T.build_k2()
    np.savez_compressed(T.K2_FIXTURE, **k2)
    k3 = T.build_k3()
    np.savez_compressed(T.K3_FIXTURE, **k3)
    for path in (T.K2_FIXTURE, T.K3_FIXTURE):
        print('%s: %d bytes' % (os.path.relpath(path), os.path.getsize(path)))


if __name__ == '__main__':
    main()
