#!/usr/bin/env python3
"""Derive the marching-cubes case table by tracing faces and write seal-3d_amd/csrc/mc_tables.h.

Numbering (shared by csrc/mesh.hip, tests/mc_witness.py and this file):
  corner c of a cell = (dx, dy, dz) with c = dx + 2 dy + 4 dz; case index = sum of (corner c solid) << c;
  edge e = 4 * axis + j runs along `axis` from its owner corner (the end with the lower coordinate), whose two other
  coordinates (a, b), in axis order, give j = a + 2 b.  EDGE_OWNER[e] is that corner, EDGE_AXIS[e] the axis.

Derivation, per case:
  * every cube face is walked counter-clockwise as seen from outside the cube.  On the walk an edge of the face is an
    ENTER edge when it goes from a non-solid to a solid corner and an EXIT edge the other way round;
  * every enter edge is joined to the exit edge that ends the run of solid corners it starts: a directed segment with the
    solid on its right.  On the ambiguous face (diagonal solid corners) this separates the two solid corners, and it uses
    nothing but the face's four corner states, so the two cells that share a face draw the same segments on it (reversed);
  * a cube edge lies on two faces that walk it in opposite directions, so it starts exactly one segment and ends exactly
    one: the segments link into closed loops;
  * each loop is fan-triangulated.  The loop is written from its lowest edge; the fan's apex is the first loop vertex for
    which no fan diagonal joins two edges of one cube face (such a diagonal could coincide with a neighbour's), else the first.
Triangles come out with their normal pointing from solid to non-solid.

    python tools/gen_mc_tables.py            rewrite csrc/mc_tables.h
    python tools/gen_mc_tables.py --print    print the header to stdout
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "seal-3d_amd", "csrc", "mc_tables.h")


def corner(dx, dy, dz):
    return dx + 2 * dy + 4 * dz


def corner_xyz(c):
    return (c & 1, (c >> 1) & 1, (c >> 2) & 1)


def _edges():
    owner, axis = [], []
    for a in range(3):
        others = [k for k in range(3) if k != a]
        for j in range(4):
            p = [0, 0, 0]
            p[others[0]], p[others[1]] = j & 1, j >> 1
            owner.append(corner(*p))
            axis.append(a)
    return owner, axis


EDGE_OWNER, EDGE_AXIS = _edges()
EDGE_ENDS = [(EDGE_OWNER[e], EDGE_OWNER[e] + (1 << EDGE_AXIS[e])) for e in range(12)]
_EDGE_OF = {frozenset(ends): e for e, ends in enumerate(EDGE_ENDS)}


def _faces():
    """six faces, each a cycle of four corners counter-clockwise as seen from outside the cube"""
    faces = []
    for a in range(3):
        u, v = (a + 1) % 3, (a + 2) % 3  # e_u x e_v = e_a
        for side in (0, 1):
            cyc = []
            for (cu, cv) in ((0, 0), (1, 0), (1, 1), (0, 1)):  # counter-clockwise about +e_a
                p = [0, 0, 0]
                p[a], p[u], p[v] = side, cu, cv
                cyc.append(corner(*p))
            if side == 0:
                cyc = cyc[::-1]  # outward normal is -e_a
            faces.append(tuple(cyc))
    return faces


FACES = _faces()
EDGE_FACES = [frozenset(f for f, cyc in enumerate(FACES) if set(EDGE_ENDS[e]) <= set(cyc)) for e in range(12)]


def case_segments(case):
    """directed segments (from edge, to edge) of one case, face by face"""
    solid = [(case >> c) & 1 for c in range(8)]
    segs = []
    for cyc in FACES:
        for k in range(4):
            if solid[cyc[k]] and not solid[cyc[k - 1]]:  # enter edge (cyc[k-1], cyc[k])
                j = k
                while solid[cyc[(j + 1) % 4]]:
                    j += 1
                segs.append((_EDGE_OF[frozenset((cyc[k - 1], cyc[k]))], _EDGE_OF[frozenset((cyc[j % 4], cyc[(j + 1) % 4]))]))
    return segs


def case_loops(case):
    nxt = {}
    for a, b in case_segments(case):
        assert a not in nxt, (case, a)
        nxt[a] = b
    assert sorted(nxt) == sorted(nxt.values()), case
    loops, seen = [], set()
    for e in sorted(nxt):
        if e in seen:
            continue
        loop = [e]
        while nxt[loop[-1]] != e:
            loop.append(nxt[loop[-1]])
        seen.update(loop)
        loops.append(loop)
    return loops


def _fan(loop):
    def diagonals_in_a_face(l):
        return sum(1 for i in range(2, len(l) - 1) if EDGE_FACES[l[0]] & EDGE_FACES[l[i]])
    best = loop
    for r in range(len(loop)):
        l = loop[r:] + loop[:r]
        if diagonals_in_a_face(l) == 0:
            best = l
            break
    return [(best[0], best[i], best[i + 1]) for i in range(1, len(best) - 1)]


def case_triangles(case):
    tris = []
    for loop in case_loops(case):
        tris.extend(_fan(loop))
    return tris


def build_tables():
    tris = [case_triangles(c) for c in range(256)]
    width = max(len(t) for t in tris)
    count = [len(t) for t in tris]
    table = []
    for t in tris:
        row = [e for tri in t for e in tri]
        table.append(row + [-1] * (3 * width - len(row)))
    return dict(width=width, count=count, table=table, edge_owner=list(EDGE_OWNER), edge_axis=list(EDGE_AXIS))


TABLES = build_tables()
MC_MAX_TRIS = TABLES["width"]
TRI_COUNT = TABLES["count"]
TRI_TABLE = TABLES["table"]


def header_text():
    t = TABLES
    out = ["// mc_tables.h - marching-cubes case tables.  GENERATED by tools/gen_mc_tables.py (face tracing); do not edit.",
           "// corner c = dx + 2 dy + 4 dz; case = sum (corner solid) << c; edge e = 4 axis + j, owned by corner MC_EDGE_OWNER[e].",
           "#pragma once",
           "#include <stdint.h>",
           "",
           f"#define MC_MAX_TRIS {t['width']}",
           "#ifndef MC_TABLE  // storage of the tables (a device file asks for constant memory)",
           "#define MC_TABLE static const",
           "#endif",
           "",
           "MC_TABLE uint8_t kMcEdgeOwner[12] = {" + ", ".join(str(v) for v in t["edge_owner"]) + "};",
           "MC_TABLE uint8_t kMcEdgeAxis[12] = {" + ", ".join(str(v) for v in t["edge_axis"]) + "};",
           "",
           "MC_TABLE uint8_t kMcTriCount[256] = {"]
    for r in range(0, 256, 32):
        out.append("    " + ", ".join(str(v) for v in t["count"][r:r + 32]) + ",")
    out += ["};", "", "// edges of the triangles of each case, three per triangle, -1 padded",
            f"MC_TABLE int8_t kMcTriTable[256][{3 * t['width']}] = {{"]
    for c in range(256):
        out.append("    {" + ", ".join(f"{v:2d}" for v in t["table"][c]) + "},")
    out += ["};", ""]
    return "\n".join(out)


def main():
    if "--print" in sys.argv[1:]:
        sys.stdout.write(header_text())
        return
    with open(HEADER, "w") as f:
        f.write(header_text())
    bad = sum(1 for c in range(256) for loop in case_loops(c)
              if any(EDGE_FACES[a] & EDGE_FACES[b] for (a, _, b) in _fan(loop)[:-1]))
    print(f"mc tables: {sum(1 for c in TRI_COUNT if c)} non-empty cases, width {MC_MAX_TRIS} triangles, "
          f"{bad} loops with a fan diagonal inside a face -> {HEADER}")


if __name__ == "__main__":
    main()
