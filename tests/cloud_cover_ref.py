"""What rrtmg_lw_hip_mcica_cloud_cover* must return, from the definitions in include/rrtmg_lw_hip.h applied to the generator's own
output: cldfmcl arrays (NG, ncol, nlay) of zeros and ones (Oracle.mcica_subcol), one per sample.  Integer counts, then ONE float64
division by NG * nsamp - numpy's float64 `/` is the IEEE division the header names.  Also the designed cloud fields of
tests/test_hip_cloud_cover.py.  No GPU, no library."""
import numpy as np


def counts(cldfmcl):
    """(lay, cum): int64 (ncol, nlay) - the sub-columns cloudy in layer k, and those cloudy in layer k or any layer above it (layer
    index 0 at the surface)"""
    c = np.asarray(cldfmcl)
    assert c.ndim == 3 and np.isin(c, (0.0, 1.0)).all(), "cldfmcl holds zeros and ones"
    c = c != 0
    lay = c.sum(axis=0, dtype=np.int64)
    seen = np.logical_or.accumulate(c[:, :, ::-1], axis=2)[:, :, ::-1]        # from the top layer down
    return lay, seen.sum(axis=0, dtype=np.int64)


def cover(samples, dtype=np.float64):
    """dict(cldtot (ncol,), cldcum, cldlay (ncol, nlay)) of the list of per-sample cldfmcl arrays: counts summed over the samples, one
    float64 division, then - for float32 - one rounding"""
    ng = samples[0].shape[0]
    lay = sum(counts(c)[0] for c in samples)
    cum = sum(counts(c)[1] for c in samples)
    den = np.float64(ng * len(samples))
    q = lambda n: np.asfortranarray((n.astype(np.float64) / den).astype(dtype))
    return {"cldtot": q(cum[:, 0]), "cldcum": q(cum), "cldlay": q(lay)}


def submask(cldfmcl):
    """uint32 (ncol, nlay, MW), MW = ceil(NG / 32): bit g % 32 of word g // 32 = cldfmcl[g]; the bits at and above NG are zero"""
    c = np.asarray(cldfmcl) != 0
    ng, ncol, nlay = c.shape
    mw = (ng + 31) // 32
    m = np.zeros((ncol, nlay, mw), dtype=np.uint32)
    for g in range(ng):
        m[:, :, g // 32] |= c[g].astype(np.uint32) << np.uint32(g % 32)
    return np.asfortranarray(m)


# ---- designed cloud fields -------------------------------------------------------------------------------------------------------------
NCOL, NLAY = 131, 13          # two 64-column blocks and a ragged tail of three; few layers: the oracle draws 131 x 13 x NG deviates per case


def _patterns(nlay):
    top, mid = nlay - 1, nlay // 2
    z = lambda: np.zeros(nlay)
    out = []

    def add(*cells):
        p = z()
        for k, v in cells:
            p[k] = v
        out.append(p)

    add()                                              # cloud-free
    add((mid, 1.0))                                    # an overcast layer: every sub-column, 128 .. NG-1 and the last mask word included
    add((4, 1e-21))                                    # below the generator's cldmin: counts as clear
    add((4, 1e-21), (9, 0.5))                          # ... beside a real cloud
    for f in (0.3, 0.7):
        add((0, f))                                    # a single layer at the surface,
        add((top, f))                                  # at the top
        add((mid, f))                                  # and mid-column
    add((5, 0.4), (6, 0.6), (7, 0.5))                  # adjacent layers
    add((0, 0.2), (1, 0.9))
    add((2, 0.5), (3, 0.3), (9, 0.2), (10, 0.6))       # two separated decks
    add((1, 0.35), (top, 0.35))
    add((3, 1.0), (8, 0.5))                            # overcast below a partial deck
    add(*[(k, 0.15) for k in range(nlay)])             # every layer
    return out


def designed_inputs(ncol=NCOL, nlay=NLAY, seed=5):
    """dict(play, cldfr, dz, lat) - (ncol, nlay) Fortran-ordered float64, lat (ncol,): the patterns above dealt over the columns in a
    shuffled order (each occurs ncol // 16 times at least), pressures that fall with height and differ in their digits from column to
    column (kissvec seeds every column's stream from its four lowest layer pressures)"""
    rng = np.random.default_rng(seed)
    pats = _patterns(nlay)
    order = rng.permutation(ncol)
    cldfr = np.zeros((ncol, nlay))
    for j, i in enumerate(order):
        cldfr[i] = pats[j % len(pats)]
    psfc = rng.uniform(960.0, 1030.0, ncol)
    edges = np.linspace(0.0, 1.0, nlay + 1)
    mids = 0.5 * (edges[:-1] + edges[1:])
    play = psfc[:, None] * (1.0 - mids[None, :]) ** 1.5 + 0.7 + rng.uniform(0.0, 0.01, (ncol, nlay))
    assert (np.diff(play, axis=1) < 0).all()
    dz = rng.uniform(100.0, 1500.0, (ncol, nlay))
    lat = rng.uniform(-90.0, 90.0, ncol)
    return {"play": np.asfortranarray(play), "cldfr": np.asfortranarray(cldfr), "dz": np.asfortranarray(dz), "lat": lat}


def oracle_cldfmcl(oracle, icld, seed, irng, play, cldfr, alpha=None):
    """the reference generator's cldfmcl (NG, ncol, nlay) for these grid-mean inputs (the water paths and optical depths do not enter the
    mask: zeros)"""
    ncol, nlay = play.shape
    z = np.zeros((ncol, nlay))
    a = z if alpha is None else alpha
    return oracle.mcica_subcol(ncol, nlay, icld, seed, irng, play, cldfr, z, z, z, z, np.zeros((16, ncol, nlay)), a)["cldfmcl"]
