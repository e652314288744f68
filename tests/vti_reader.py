"""A reader of the `-map` files (VTK XML ImageData, raw appended data with UInt64 headers) for the tests: a parser of its own,
nothing of the library.  read_vti returns the attributes of the image, the arrays of CellData and FieldData in file order and
the raw bytes."""
import re
import struct

import numpy as np

DTYPES = {"Float64": "<f8", "Int32": "<i4", "Int64": "<i8", "UInt8": "u1"}


def _attrs(tag):
    return dict(re.findall(r'(\w+)="([^"]*)"', tag))


def read_vti(path):
    raw = open(path, "rb").read()
    mark = raw.index(b'<AppendedData encoding="raw">\n_')
    head = raw[:mark].decode("ascii")
    data = raw[mark + len(b'<AppendedData encoding="raw">\n_'):]
    assert raw.endswith(b"\n</AppendedData>\n</VTKFile>\n")
    data = data[:-len(b"\n</AppendedData>\n</VTKFile>\n")]
    lines = head.splitlines()
    assert lines[0] == '<?xml version="1.0"?>'
    vtk = _attrs(lines[1])
    assert lines[1].startswith("<VTKFile ") and vtk == dict(type="ImageData", version="1.0", byte_order="LittleEndian", header_type="UInt64")
    image = _attrs(next(l for l in lines if l.startswith("<ImageData ")))
    piece = _attrs(next(l for l in lines if l.startswith("<Piece ")))
    out = dict(whole_extent=[int(x) for x in image["WholeExtent"].split()], origin=[float(x) for x in image["Origin"].split()],
               spacing=[float(x) for x in image["Spacing"].split()], piece_extent=[int(x) for x in piece["Extent"].split()], raw=raw,
               field={}, cell={}, field_order=[], cell_order=[], types={})
    section, expect = None, 0
    for l in lines:
        if l.startswith("<FieldData"):
            section = "field"
        elif l.startswith("<CellData"):
            section = "cell"
            out["cell_attrs"] = _attrs(l)
        elif l.startswith("</FieldData") or l.startswith("</CellData"):
            section = None
        elif l.startswith("<DataArray "):
            a = _attrs(l)
            assert section is not None and a["format"] == "appended" and int(a["offset"]) == expect, l
            nbytes = struct.unpack_from("<Q", data, expect)[0]
            arr = np.frombuffer(data, dtype=DTYPES[a["type"]], count=nbytes // np.dtype(DTYPES[a["type"]]).itemsize, offset=expect + 8)
            ncomp = int(a.get("NumberOfComponents", "1"))
            if "NumberOfTuples" in a:
                assert arr.size == int(a["NumberOfTuples"])
            out[section][a["Name"]] = arr.reshape(-1, ncomp) if ncomp > 1 else arr
            out[section + "_order"].append(a["Name"])
            out["types"][a["Name"]] = a["type"]
            expect += 8 + nbytes
    assert expect == len(data), "bytes behind the last array"
    return out
