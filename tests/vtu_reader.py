"""A reader of the .vtu files of the `-paraview` dumps for the tests: the XML header by regular expressions, the raw
appended blocks (UInt64 byte count, then the data, little endian) with numpy.  Knows nothing of the writer."""
import re

import numpy as np

_DTYPES = {"Float64": "<f8", "Float32": "<f4", "Int64": "<i8", "Int32": "<i4", "UInt8": "u1", "UInt64": "<u8"}


def read_vtu(path):
    """dict(attrs = attributes of <VTKFile>, npoints, ncells, arrays = name -> numpy array (tuples x components for
    vectors), types = name -> VTK type name, ncomp = name -> components)"""
    raw = open(path, "rb").read()
    marker = b'<AppendedData encoding="raw">'
    cut = raw.index(marker)
    head = raw[:cut].decode("ascii")
    start = raw.index(b"_", cut + len(marker)) + 1
    assert raw.rstrip().endswith(b"</VTKFile>") and b"</AppendedData>" in raw[start:]
    attrs = dict(re.findall(r'(\w+)="([^"]*)"', re.search(r"<VTKFile([^>]*)>", head).group(1)))
    assert attrs["type"] == "UnstructuredGrid"
    piece = re.search(r'<Piece NumberOfPoints="(\d+)" NumberOfCells="(\d+)"', head)
    out = dict(attrs=attrs, npoints=int(piece.group(1)), ncells=int(piece.group(2)), arrays={}, types={}, ncomp={})
    section = {}
    for sec in ("FieldData", "Points", "Cells", "PointData", "CellData"):
        m = re.search(rf"<{sec}[ >].*?</{sec}>", head, flags=re.S)
        assert m, sec
        for el in re.findall(r"<DataArray([^>]*)/>", m.group(0)):
            a = dict(re.findall(r'(\w+)="([^"]*)"', el))
            assert a["format"] == "appended"
            section[a["Name"]] = sec
            off = start + int(a["offset"])
            nbytes = int(np.frombuffer(raw, dtype="<u8", count=1, offset=off)[0])
            dt = np.dtype(_DTYPES[a["type"]])
            assert nbytes % dt.itemsize == 0
            arr = np.frombuffer(raw, dtype=dt, count=nbytes // dt.itemsize, offset=off + 8)
            nc = int(a.get("NumberOfComponents", 1))
            out["arrays"][a["Name"]] = arr.reshape(-1, nc) if nc > 1 else arr
            out["types"][a["Name"]] = a["type"]
            out["ncomp"][a["Name"]] = nc
    # sizes the header promises
    for name, sec in section.items():
        n = out["arrays"][name].shape[0]
        if sec in ("Points", "PointData"):
            assert n == out["npoints"], name
        elif sec == "CellData" or name in ("offsets", "types"):
            assert n == out["ncells"], name
    out["section"] = section
    return out
