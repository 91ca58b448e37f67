"""The renderer's proto reader (video_segment_amd/render/render_desc.h) on bytes it must not trust, on the CPU.

tests/host/desc_reader_harness.cpp includes the reader as libvsg_render's one translation unit does and is built
with the host's address and undefined-behaviour sanitizers.  For three SegmentationDescs of an 8 x 6 frame it parses
the desc, every prefix of it and every replacement of one byte by 0x00, 0x7f, 0x80 and 0xff, and runs what the
library runs on a desc before any device work: IsVectorOnly, ParseDesc, ParentId of every region at every level
and, for a vector-only desc, BuildLines.  Every input has to parse or to be refused as VSG_ERR_INVALID, with no
sanitizer report; the intact descs have to give the regions, intervals, hierarchy and lines written down here."""
import os
import re
import struct
import subprocess

import pytest

import vector_cases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 8, 6


def _varint(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7f) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def _int(number, value):
    return _varint(number << 3) + _varint(value)


def _bytes(number, payload):
    return _varint(number << 3 | 2) + _varint(len(payload)) + payload


# id -> scan intervals (y, left_x, right_x); together they cover the frame
RASTERS = {1: [(0, 0, 3), (1, 0, 3)],
           2: [(0, 4, 7), (1, 4, 7), (2, 0, 7)],
           5: [(3, 0, 7), (4, 0, 7), (5, 0, 7)]}
# two levels: (id, parent_id) sorted by id
HIERARCHY = [[(1, 10), (2, 10), (5, 11)], [(10, None), (11, None)]]


def _hierarchy():
    out = b""
    for level in HIERARCHY:
        regions = b"".join(_bytes(2, _int(1, rid) + (_int(4, parent) if parent is not None else b""))
                           for rid, parent in level)
        out += _bytes(3, regions)                                           # SegmentationDesc.hierarchy
    return out


def raster_desc():
    out = b""
    for rid, scans in RASTERS.items():
        raster = b"".join(_bytes(1, _int(1, y) + _int(2, lx) + _int(3, rx)) for y, lx, rx in scans)
        out += _bytes(2, _int(1, rid) + _bytes(3, raster))                  # region: id, raster
    return out + _int(4, W) + _int(5, H) + _hierarchy()


def _rect(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1), (x0, y0)]


def vector_desc():
    """The regions of raster_desc() as rectangles, vector-only: coord_idx packed (region 1), unpacked (region 2)
    and both in one polygon (region 5); VectorMesh.coord half packed, half unpacked."""
    polygons = {1: _rect(0, 0, 4, 2), 2: _rect(4, 0, 8, 2), 5: _rect(0, 3, 8, 6)}
    coord, out = [], b""
    for rid, pts in polygons.items():
        idx = []
        for x, y in pts:
            idx.append(len(coord))
            coord += [float(x), float(y)]
        packed = _bytes(1, b"".join(_varint(i) for i in idx))
        unpacked = b"".join(_int(1, i) for i in idx)
        mixed = b"".join(_int(1, i) for i in idx[:2]) + _bytes(1, b"".join(_varint(i) for i in idx[2:]))
        polygon = {1: packed, 2: unpacked, 5: mixed}[rid]
        out += _bytes(2, _int(1, rid) + _bytes(6, _bytes(1, polygon)))      # region: id, vectorization.polygon
    half = len(coord) // 2
    mesh = _bytes(1, struct.pack("<%df" % half, *coord[:half]))
    mesh += b"".join(_varint(1 << 3 | 5) + struct.pack("<f", c) for c in coord[half:])
    return out + _int(4, W) + _int(5, H) + _hierarchy() + _bytes(11, mesh) + _int(13, 1)


def library_vector_desc():
    """Two rectangles as the tests of the vector path make them."""
    return vc.make_desc(W, H, [(3, [vc.rect(0, 0, 8, 3)]), (4, [vc.rect(0, 3, 8, 6)])]).SerializeToString()


# name -> (bytes, region ids, intervals per region, hierarchy level sizes, polygon lines or -1).  A rectangle has
# two lines that are not horizontal.
CASES = {
    "raster": (raster_desc, [1, 2, 5], [2, 3, 3], [3, 2], -1),
    "vector": (vector_desc, [1, 2, 5], [0, 0, 0], [3, 2], 6),
    "library_vector": (library_vector_desc, [3, 4], [0, 0], [], 4),
}


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("desc_reader") / "desc_reader_harness")
    subprocess.run(["hipcc", "-x", "hip", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17",
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "host", "desc_reader_harness.cpp"), "-o", exe],
                   check=True, timeout=300)
    return exe


def _run(args):
    r = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
    return r.stdout


def _list(values):
    return ",".join(str(v) for v in values) or "-"


def test_empty_packed_mesh_coordinates(harness, tmp_path):
    """A packed VectorMesh.coord of no bytes, first in its mesh: the reader handed memcpy the null data() of its
    empty coordinate vector.  The desc has no region and parses."""
    path = tmp_path / "empty_coord.pb"
    path.write_bytes(_bytes(11, _bytes(1, b"")) + _int(13, 1))
    assert "one: parsed" in _run([harness, "one", str(path), str(W), str(H)])


@pytest.mark.parametrize("name", sorted(CASES))
def test_reader_parses_or_refuses_every_prefix_and_mutation(harness, tmp_path, name):
    make, ids, intervals, levels, lines = CASES[name]
    desc = make()
    # the first field is a region (tag 0x12, a length of one byte): three bytes end inside its payload
    assert desc[0] == 0x12 and 2 <= desc[1] < 0x80
    path = tmp_path / (name + ".pb")
    path.write_bytes(desc)
    out = _run([harness, "sweep", str(path), str(W), str(H), "3", _list(ids), _list(intervals), _list(levels),
                str(lines)])
    print(out)
    assert "intact: regions=%d" % len(ids) in out
    prefixes = re.search(r"prefixes: parsed=(\d+) rejected=(\d+)", out)
    mutations = re.search(r"mutations: parsed=(\d+) rejected=(\d+)", out)
    assert prefixes and int(prefixes.group(1)) > 0 and int(prefixes.group(2)) > 0
    assert int(prefixes.group(1)) + int(prefixes.group(2)) == len(desc) + 1
    # 0x7f or 0xff in a length or a wire type breaks the message; 0x00 in an interval's x does not
    assert mutations and int(mutations.group(1)) > 0 and int(mutations.group(2)) > 0
    assert 3 * len(desc) <= int(mutations.group(1)) + int(mutations.group(2)) <= 4 * len(desc)
