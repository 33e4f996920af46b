"""Contour levels for the pairwise posterior plots: ``find_levels`` of ``ces/plots.py`` (:7-33).

Only ``find_levels`` is here; it needs numpy alone.  ``plot_kde`` and ``abline`` of the reference draw with seaborn and
stay out.

Build-only extra: kwarg ``H`` -- a 2-D histogram that is already there, such as
``MCMC.marginals['hist2d'][k]`` of ``model_mh`` / ``gp_mh`` with ``chains=M, summary=True, marginals=...`` -- so that the
levels come without the samples: ``find_levels(H=m.marginals['hist2d'][0])``.
"""
import numpy as np


def find_levels(x=None, y=None, contours=[.9999, .99, .95, .68], H=None, energy=None):
    """The histogram levels whose super-level sets hold the masses ``contours``, then ``H.max()`` (ces/plots.py:7-33).

    The histogram is, in this order, ``exp(-energy)``, ``H``, or the 20 x 20 density histogram of the samples ``x, y``
    (the reference asks numpy for ``normed=True``, which numpy no longer has: ``density=True`` is the same histogram).
    For every contour c a bisection between ``H.min()`` and ``H.max()`` finds where ``H[H > level].sum() - c H.sum()`` changes
    sign, as the reference's ``scipy.optimize.bisect`` does.  That function is a step in ``level``, and the bisection here
    runs until the bracket is one floating-point number wide and returns its upper end: the level is a cell value v with
    ``H[H > v].sum() <= c H.sum() < H[H >= v].sum()``.  As in the reference, a contour whose bracket has no change of
    sign (the cells at ``H.min()`` alone hold more than 1 - c of the mass) raises ``ValueError``.
    Returns the list of levels (``len(contours) + 1``); with ``energy=``, ``-log(levels)[::-1]`` as an array."""
    if energy is not None:
        H = np.exp(-np.asarray(energy, dtype=np.float64))
    elif H is not None:
        H = np.asarray(H, dtype=np.float64)
    else:
        if x is None or y is None:
            raise ValueError("find_levels needs the samples x and y, a histogram H= or energy=")
        H = np.histogram2d(x, y, bins=20, density=True)[0]
    norm = H.sum()
    lo0, hi0 = float(H.min()), float(H.max())

    def objective(limit, target):
        return H[H > limit].sum() - target

    levels = []
    for c in contours:
        target = norm * c
        lo, hi = lo0, hi0
        if not (objective(lo, target) > 0 >= objective(hi, target)):
            raise ValueError("find_levels: no level between H.min() and H.max() holds the mass %r: the objective has the "
                             "same sign at both ends" % (c,))
        while True:
            mid = lo + 0.5 * (hi - lo)
            if not lo < mid < hi:
                break
            if objective(mid, target) > 0:
                lo = mid
            else:
                hi = mid
        levels.append(hi)
    levels.append(hi0)                                    # the top level, for the shading of a filled contour plot
    if energy is None:
        return levels
    return -np.log(levels)[::-1]
