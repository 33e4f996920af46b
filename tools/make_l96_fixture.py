"""Write tests/golden/l96_long.npz: the host's mean and standard deviation of the 25 window statistics of a (5, 3) two-scale
Lorenz '96 model over 64 particles from perturbed on-attractor starts (tests/test_gpu_l96.py::test_long_window_in_distribution
compares the device's 1024-particle ensemble with it in distribution).

    python tools/make_l96_fixture.py

Everything comes from the repo's own host model (ces_amd/models.py: solve + statistics); the seeds are fixed.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import l96_cases as lc  # noqa: E402

SHAPE, T, N_HOST = (5, 3), 4.0, 64
HOST_SEED, DEVICE_SEED = 21, 22
OUT = os.path.join(ROOT, "tests", "golden", "l96_long.npz")


def model(device=False):
    return lc.make_model("lorenz96", SHAPE, T=T, dt=0.1, device=device, l_window=2, freq=10, spinup=2)


def times():
    return np.linspace(0.0, T, 41)


def starts(n, seed):
    """(n_state, n): the on-attractor state of tests/l96_cases.py times 1 + 0.05 N(0, 1), elementwise."""
    w = lc.attractor_state(*SHAPE)
    return w[:, None] * (1.0 + 0.05 * np.random.RandomState(seed).standard_normal((w.size, n)))


def main():
    m, t, W = model(), times(), starts(N_HOST, HOST_SEED)
    G = np.stack([m.statistics(m.solve(W[:, j], t, args=tuple(lc.PAR_MEAN))) for j in range(N_HOST)], axis=1)
    np.savez(OUT, mean=G.mean(axis=1), sd=G.std(axis=1, ddof=1), n=np.int64(N_HOST))
    print(OUT, G.shape, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
