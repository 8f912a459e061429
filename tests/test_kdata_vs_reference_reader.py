"""kdata.from_netcdf against the reference's OWN netCDF reader.

The converter's earlier test wrote its file with a mirror of the converter, so a misread of the reader - dimension order, absorber
index, gPointSetNumber - would have passed.  tests/golden/ref_nc_reads.json holds every read the reference's src/rrtmg_lw_read_nc.f90
makes (tools/gen_nc_reads.py parses its `nf90_inq_varid` / `nf90_get_var(..., start = (/.../), count = (/.../))` /
`getAbsorberIndex` statements and the dimension parameters of modules/rrlw_ncpar.f90), and every read is carried out on a synthetic
file of distinct random numbers with nf90_get_var's semantics: the hyperslab start / count in Fortran dimension order (the reverse of
the file's C order), its elements assigned to the target array in array-element order.  Sixteen bands, every array of kspec.KSPEC:
from_netcdf must return exactly those numbers.
"""
import json
import os

import numpy as np

from rrtmg_lw_amd.kdata import from_netcdf
from rrtmg_lw_amd.kspec import KSPEC, blob_name, shape_of

FIX = os.path.join(os.path.dirname(__file__), "golden", "ref_nc_reads.json")


def _fixture():
    """(dimension sizes by name, [(band, target, variable, start, count)])"""
    f = json.load(open(FIX))
    return f["dims"], [tuple(r) for r in f["reads"]]


def _write_file(path, rng, dims):
    from scipy.io import netcdf_file
    f = netcdf_file(path, "w")
    for n, s in dims.items():
        f.createDimension(n, s)
    # C order = the reverse of the reader's Fortran order, Appendix D of SURVEY.md
    layout = {
        "PlanckFractionLowerAtmos": ("GPointSet", "band", "keylower", "GPoint"),
        "PlanckFractionUpperAtmos": ("GPointSet", "band", "keyupper", "GPoint"),
        "KeySpeciesAbsorptionCoefficientsLowerAtmos": ("GPointSet", "band", "GPoint", "plower", "Tdiff", "keylower"),
        "KeySpeciesAbsorptionCoefficientsUpperAtmos": ("GPointSet", "band", "GPoint", "pupper", "Tdiff", "keyupper"),
        "H20SelfAbsorptionCoefficients": ("GPointSet", "band", "GPoint", "Tself"),
        "H20ForeignAbsorptionCoefficients": ("GPointSet", "band", "GPoint", "Tforeign"),
        "AbsorptionCoefficientsLowerAtmos": ("GPointSet", "band", "Absorber", "GPoint", "T", "keylower"),
        "AbsorptionCoefficientsUpperAtmos": ("GPointSet", "band", "Absorber", "GPoint", "T", "keyupper"),
    }
    data = {}
    for n, d in layout.items():
        v = f.createVariable(n, "d", d)
        a = rng.random(tuple(dims[x] for x in d))
        v[:] = a
        data[n] = a
    f.close()
    return data


def test_converter_agrees_with_the_reference_reader(tmp_path):
    dims, reads = _fixture()
    assert len(reads) == sum(len(v) for v in KSPEC.values())             # one nf90_get_var per array of every band
    path = str(tmp_path / "rrtmg_lw.nc")
    data = _write_file(path, np.random.default_rng(20240607), dims)
    got = from_netcdf(path)
    seen = set()
    for band, target, var, start, count in reads:
        bounds = {n: b for n, b, _, _ in KSPEC[band]}[target]
        shp = shape_of(bounds)
        vf = data[var].transpose()                                         # Fortran index order
        assert len(start) == len(count) == vf.ndim, (band, target)
        slab = vf[tuple(slice(s - 1, s - 1 + c) for s, c in zip(start, count))]
        assert slab.shape == tuple(count) and slab.size == int(np.prod(shp)), (band, target, count, shp)
        want = slab.flatten(order="F").reshape(shp, order="F")            # nf90_get_var fills the target in array-element order
        a = got[blob_name(band, target)]
        assert a.shape == shp and np.array_equal(a, want), (band, target, var, start, count)
        seen.add((band, target))
    assert seen == {(b, n) for b in KSPEC for n, _, _, _ in KSPEC[b]}
