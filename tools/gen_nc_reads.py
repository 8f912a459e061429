#!/usr/bin/env python3
"""Write tests/golden/ref_nc_reads.json: every hyperslab read of the reference's own netCDF reader, for
tests/test_kdata_vs_reference_reader.py.

The statements of src/rrtmg_lw_read_nc.f90 are parsed where they lie (`nf90_inq_varid(ncid, "Variable", varID)`,
`nf90_get_var(ncid, varID, target, start = (/.../), count = (/.../))`, `call getAbsorberIndex('GAS', ab)`), with the
dimension parameters and the absorber list of modules/rrlw_ncpar.f90.  The fixture holds numbers only: the file's
dimension sizes and one [band, target, variable, start, count] per read (start / count in Fortran dimension order,
every name resolved to an integer).

Run:  python tools/gen_nc_reads.py <reference root>
"""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "ref_nc_reads.json")
DIMS = ("GPointSet", "band", "GPoint", "keylower", "keyupper", "Tdiff", "plower", "pupper", "Tself", "Tforeign", "T", "Absorber")


def _join_continuations(text):
    text = re.sub(r"!.*", "", text)                       # comments
    return re.sub(r"&\s*\n\s*&?", " ", text)


def _ncpar(ncpar):
    t = _join_continuations(open(ncpar).read())
    par = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"\b(\w+)\s*=\s*(\d+)\b", t)}
    names = [n.strip() for n in re.findall(r"'([A-Za-z0-9 ]+)'", t[t.index("AbsorberNames"):t.index("/)")])]
    assert len(names) == par["absorber"] == 12
    return par, names


def _reads(reader, ncpar):
    """[(band, target, variable, start, count)] with start / count as lists of integers (Fortran order)"""
    par, absorbers = _ncpar(ncpar)
    t = _join_continuations(open(reader).read())
    out = []
    for m in re.finditer(r"subroutine\s+lw_kgb(\d\d)\b(.*?)end\s+subroutine", t, flags=re.S | re.I):
        band, body = int(m.group(1)), m.group(2)
        env = dict(par)
        for pm in re.finditer(r"parameter\s*::\s*(.*)", body):
            for a in pm.group(1).split(","):
                k, _, v = a.partition("=")
                v = v.strip()
                env[k.strip().lower()] = 16 if re.fullmatch(r"no\d+", v) else int(v)      # no1 .. no16 = 16 (modules/rrlw_kgNN.f90)
        assert env["bandnumber"] == band and env["gpointsetnumber"] == 1
        var = None
        for st in re.finditer(r"getAbsorberIndex\('(\w+)'\s*,\s*ab\)|nf90_inq_varid\(ncid,\s*\"(\w+)\"|"
                              r"nf90_get_var\(ncid,\s*varID,\s*(\w+)(?:\([^)]*\))?,\s*start\s*=\s*\(/(.*?)/\)\s*,\s*count\s*=\s*\(/(.*?)/\)\)", body):
            if st.group(1):
                env["ab"] = absorbers.index(st.group(1)) + 1
            elif st.group(2):
                var = st.group(2)
            else:
                ev = lambda s: [int(x) if x.isdigit() else env[x.lower()] for x in (y.strip().replace("_im", "") for y in s.split(","))]
                out.append((band, st.group(3).lower(), var, ev(st.group(4)), ev(st.group(5))))
    return par, out


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__.strip().splitlines()[-1])
    ref = sys.argv[1]
    par, reads = _reads(os.path.join(ref, "src", "rrtmg_lw_read_nc.f90"), os.path.join(ref, "modules", "rrlw_ncpar.f90"))
    with open(OUT, "w") as f:
        json.dump(dict(dims={n: par[n.lower()] for n in DIMS}, reads=reads), f, separators=(",", ":"))
        f.write("\n")
    print(f"{OUT}: {len(reads)} reads")


if __name__ == "__main__":
    main()
