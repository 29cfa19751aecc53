"""CPU: the WKT ingest contract (gf_wkt_parse_geoms, gf_wkt_parse_points).

The device's per-line evaluator (spatialflink_amd/csrc/gf_wkt_geom.hpp), built for the host under the
sanitizers as a stand-alone program (tests/native/wktingest_main.cpp), agrees with the independent
restatement (tests/wktingest_ref.py) on every generated, bad and unsupported line, vertex bits
included; pass A alone accepts whatever the whole contract accepts; the windows are those of the host
mirror's Polygon / LineString; the same geometries written as GeoJSON give the same rings and bits
through tests/geomingest_ref.py; the dispatchers refuse unknown input types."""
import os
import struct
import subprocess

import pytest

import spatialflink_amd as sf
from spatialflink_amd.spatialStreams import Deserialization as D

import geomingest_ref as GR
import wktingest_gen as W
import wktingest_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = (W.POINT, W.POLYGON, W.LINESTRING)
# (delimiter, date format) of the maps: the non-T ones, then T variants
SCHEMAS = ((None, 0), (",", 1), (";", 0), ("\t", 1))


def _kw(delim, df):
    return dict(delimiter=delim.encode() if delim else None, date_fmt=df)


@pytest.fixture(scope="module")
def generated():
    """every generated line with the restatement's verdict; none may be refused"""
    got = {}
    for kind in KINDS:
        for si, (delim, df) in enumerate(SCHEMAS):
            rows = []
            for ln in W.corpus(kind, 90, 21 + si, delim, bool(df), big_every=45 if kind != W.POINT else 0):
                r, k = R.wkt_line(ln, kind, **_kw(delim, df))
                assert k == 0, (kind, k, ln[:300])
                rows.append((ln, r))
            got[kind, delim, df] = rows
    return got


def test_generator_covers_what_it_promises(generated):
    for kind in KINDS:
        lines = [ln for (k, *_), rows in generated.items() if k == kind for ln, _ in rows]
        assert any(b"\t" in ln for ln in lines) and any(b'{"key"' in ln for ln in lines)
        assert any(b"e-3" in ln for ln in lines) and any(b"-0" in ln for ln in lines) and any(b"(+" in ln or b" +" in ln for ln in lines)
        if kind == W.POINT:
            continue
        assert any(b"MULTI" in ln for ln in lines) and any(b"MULTI" not in ln for ln in lines)
        objs = [r[0] for (k, *_), rows in generated.items() if k == kind for _, r in rows]
        sizes = [len(c) for o in objs for c in (o if kind == W.POLYGON else [o])]
        assert max(sizes) == 4097 and min(sizes) == (4 if kind == W.POLYGON else 2)
        rows = generated[kind, ",", 1]
        assert any(r[1] is None for _, r in rows) and any(r[1] is not None for _, r in rows)
        assert any(r[2] == 0 for _, r in rows) and any(r[2] != 0 for _, r in rows)
    polys = [r[0] for _, r in generated[W.POLYGON, None, 0]]
    assert {len(p) for p in polys} >= {1, 2, 3, 4}
    assert any(a == b for p in polys for a, b in zip(p[:-1], p[1:])), "two identical rings"
    assert any(GR.ring_area(p[0]) > GR.ring_area(p[-1]) for p in polys if len(p) > 1)


def test_the_references_own_samples():
    r, k = R.wkt_line(W.SAMPLE_POLYGON, W.POLYGON)
    assert k == 0 and len(r[0]) == 1 and len(r[0][0]) == 9 and r[0][0][0] == (-74.15010482037168, 40.62183511874645)
    assert R.wkt_line(W.SAMPLE_LINESTRING, W.LINESTRING) == (None, R.MISSING)


def test_bad_and_unsupported_lines_have_their_kinds():
    for kind, ln, want in W.BAD:
        assert R.wkt_line(ln, kind) == (None, want), (want, ln)
    for kind, ln in W.UNSUPPORTED:
        assert R.wkt_line(ln, kind) == (None, R.UNSUPPORTED), ln
    assert R.wkt_line(b"", W.POLYGON)[1] == R.EMPTY


T_LINES = W.T_LINES


def test_objid_and_time_rules_of_the_restatement():
    got = [R.wkt_line(ln, kind, **_kw(d, df)) for kind, ln, d, df in T_LINES]
    oid_ts = [(r[1], r[2]) if r else k for r, k in got]
    t = 1577934245000
    assert oid_ts[:8] == [(b"7", t), (None, 0), (None, 0), (b"7", 0), (b"veh-1", 0), (b"veh-1", 0), (None, t), (None, t)]
    assert oid_ts[8] == (b"7", 1609556645000) and oid_ts[9] == (b"007", t) and oid_ts[10] == (b"", t)
    assert oid_ts[11] == (b"a b", t) and oid_ts[12][0] == b"-12" and oid_ts[13:] == [R.UNSUPPORTED, R.MISSING]


def test_same_rings_as_the_host_mirror_and_as_the_geojson_ingest():
    for kind in (W.POLYGON, W.LINESTRING):
        for ln, (members, multi) in W.corpus(kind, 60, 5, json_safe=True, with_geoms=True, big_every=30):
            r, k = R.wkt_line(ln, kind)
            assert k == 0
            plain = [[(float(x), float(y)) for x, y in c] for c in (members[0] if kind == W.POLYGON else members[:1])]
            if kind == W.POLYGON:
                assert sf.Polygon(plain).rings == r[0]
            else:
                assert sf.LineString(plain[0]).coordinates == r[0]
            g, gk = GR.geom_line(W.geojson_twin(kind, members, multi), kind, value_lines=True)
            assert gk == 0 and g[0] == r[0]
            assert [struct.pack("<d", v) for c in (g[0] if kind == W.POLYGON else [g[0]]) for p in c for v in p] == \
                   [struct.pack("<d", v) for c in (r[0] if kind == W.POLYGON else [r[0]]) for p in c for v in p]


def test_dispatchers():
    assert isinstance(D.PolygonStream("WKT"), D.WKTToSpatialPolygon)
    assert isinstance(D.PolygonStream("GeoJSON"), D.GeoJSONToSpatialPolygon)
    assert isinstance(D.LineStringStream("WKT"), D.WKTToSpatialLineString)
    assert isinstance(D.TrajectoryStreamPolygon("WKT", "yyyy-MM-dd HH:mm:ss", ";"), D.WKTToTSpatialPolygon)
    assert isinstance(D.TrajectoryStreamLineString("WKT", None, ","), D.WKTToTSpatialLineString)
    assert isinstance(D.TrajectoryStreamLineString("GeoJSON", None, ",", "t", "oid"), D.GeoJSONToTSpatialLineString)
    assert isinstance(D.PointStream("WKT"), D.WKTToSpatial)
    assert isinstance(D.TrajectoryStream("WKT"), D.WKTToTSpatial)
    assert isinstance(D.TrajectoryStream("CSV"), D.CSVTSVToTSpatial) and isinstance(D.TrajectoryStream("TSV", delimiter="\t"), D.CSVTSVToTSpatial)
    assert isinstance(D.TrajectoryStream("GeoJSON"), D.GeoJSONToTSpatial)
    for fn in (D.PolygonStream, D.LineStringStream, D.TrajectoryStreamPolygon, D.TrajectoryStreamLineString):
        for bad in ("CSV", "wkt", "", "TSV"):
            with pytest.raises(ValueError, match=f"inputType : {bad} is not support"):
                fn(bad)
    for t in ("GeoJSON", "CSV", "TSV"):
        with pytest.raises(ValueError, match="Not yet support"):
            D.PointStream(t)


# ---- the device's evaluator, on the host, under the sanitizers ------------------------------------------
@pytest.fixture(scope="module")
def native(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("wktingest") / "wktingest_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I/opt/rocm/include",
                    "-D__HIP_PLATFORM_AMD__", os.path.join(ROOT, "tests", "native", "wktingest_main.cpp"), "-o", exe],
                   check=True)
    return exe


def _run_native(exe, tmp_path, lines, kind, delim=None, df=0, tz=0):
    src = tmp_path / "lines.txt"
    src.write_bytes(b"\n".join(lines) + b"\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    run = subprocess.run([exe, str(src), str(kind), str(ord(delim) if delim else 0), str(df), str(tz)],
                         capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stderr[-3000:]
    rows = run.stdout.splitlines()
    assert len(rows) == len(lines)
    return rows


def _bits(v):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", v))[0]


def _check_row(row, ref, kind, ln):
    r, k = ref
    f = row.split(" ")
    assert int(f[0]) == k, (f[:2], k, ln[:300])
    if k:
        return
    obj, oid, ts = r
    chains = obj if kind == W.POLYGON else [obj] if kind == W.LINESTRING else [[obj]]
    nr, nv = int(f[2]), int(f[3])
    assert nr == (len(obj) if kind == W.POLYGON else 0) and nv == sum(len(c) for c in chains)
    assert int(f[4]) == ts
    if oid is None:
        assert f[5] == "null"
    elif f[5].startswith("k:"):
        assert f[5][2:].encode() == oid
    else:
        assert f[5] == "s:" + oid.hex()
    bar = f.index("|")
    assert [int(x) for x in f[6:bar]] == ([len(c) for c in chains] if kind == W.POLYGON else [])
    want = [b for c in chains for p in c for b in (_bits(p[0]), _bits(p[1]))]
    assert f[bar + 1:] == want, ln[:300]


@pytest.mark.parametrize("kind", KINDS)
def test_native_evaluator_equals_the_restatement_on_generated_lines(kind, native, generated, tmp_path):
    for (k, delim, df), rows in generated.items():
        if k != kind:
            continue
        out = _run_native(native, tmp_path, [ln for ln, _ in rows], kind, delim, df)
        for row, (ln, r) in zip(out, rows):
            _check_row(row, (r, 0), kind, ln)
            assert row.split(" ")[1] == "0"  # pass A alone accepts what the whole contract accepts


def test_native_evaluator_equals_the_restatement_on_bad_and_unsupported_lines(native, tmp_path):
    for kind in KINDS:
        lines = [ln for k, ln, _ in W.BAD if k == kind] + [ln for k, ln in W.UNSUPPORTED if k == kind]
        lines += [b"", b"   ", b"\r", W.SAMPLE_POLYGON, W.SAMPLE_LINESTRING, b"xPOINT(1 2)POLYGON((0 0,1 0,1 1,0 0))LINESTRING(0 0,1 1)"]
        out = _run_native(native, tmp_path, lines, kind)
        for row, ln in zip(out, lines):
            _check_row(row, R.wkt_line(ln, kind), kind, ln)
        # pass A alone refuses nothing the whole contract takes, and lets only unclosed rings through
        for row, ln in zip(out, lines):
            st, sta = (int(x) for x in row.split(" ")[:2])
            assert (st == 0 and sta == 0) or (st != 0 and (sta != 0 or b"POLYGON" in ln)), row


def test_native_evaluator_equals_the_restatement_on_the_objid_and_time_rules(native, tmp_path):
    for kind, ln, d, df in T_LINES:
        for tz in (0, 540):
            row = _run_native(native, tmp_path, [ln], kind, d, df, tz)[0]
            _check_row(row, R.wkt_line(ln, kind, tz_off_min=tz, **_kw(d, df)), kind, ln)
