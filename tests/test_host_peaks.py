"""`-peaks` on the host, no GPU: what the command line refuses before anything touches the GPU (the `laghos` executable, as
tests/test_host_faces.py runs it), and the sidecar of a checkpoint piece (laghos_amd/host/records_sidecar.cpp) through its
write, read and match probes: the round trip to the bit, and each corruption refused with its own message naming the file."""
import os

import numpy as np
import pytest

import test_host_faces
from records_ref import bits

# (extra options, mesh, words of the message) in the form of test_host_faces.BAD
BAD = {
    "no-material-dump": (["-peaks", "1"], "cube01_hex", "-peaks", "-paraview, -pv-surface or -pv-slice"),
    "contours-are-not-material": (["-peaks", "1", "-pv-iso", "density", "1.5"], "cube01_hex", "-peaks", "-paraview, -pv-surface or -pv-slice"),
    "arrival-alone": (["-paraview", "-peaks-arrival", "0.5"], "cube01_hex", "-peaks-arrival", "needs -peaks"),
    "N-zero": (["-paraview", "-peaks", "0"], "cube01_hex", "-peaks", "at least 1", "got 0"),
    "N-negative": (["-paraview", "--peaks-steps", "-2"], "cube01_hex", "-peaks", "at least 1", "got -2"),
    "N-word": (["-paraview", "-peaks", "often"], "cube01_hex", "-peaks", "at least 1", "got often"),
    "no-N": (["-paraview", "-peaks"], "cube01_hex", "-peaks", "missing value"),
    "threshold-inf": (["-paraview", "-peaks", "1", "-peaks-arrival", "inf"], "cube01_hex", "-peaks-arrival", "finite", "inf"),
    "threshold-nan": (["-paraview", "-peaks", "1", "--peaks-arrival", "nan"], "cube01_hex", "-peaks-arrival", "finite", "nan"),
    "threshold-half-a-number": (["-paraview", "-peaks", "1", "-peaks-arrival", "0.5bar"], "cube01_hex", "-peaks-arrival", "finite number", "0.5bar"),
    "no-threshold": (["-pv-surface", "-peaks", "1", "-peaks-arrival"], "cube01_hex", "-peaks-arrival", "missing value"),
    "1D-faces": (["-pv-surface", "-peaks", "1"], "segment01", "-pv-surface", "1D"),
}


@pytest.mark.parametrize("case", list(BAD))
def test_driver_refuses_bad_peaks_options_before_the_gpu(case, tmp_path, monkeypatch):
    """(the refusal comes before the first call of the GPU runtime: the executable gives it on a machine without a GPU too)"""
    monkeypatch.setitem(test_host_faces.BAD, case, BAD[case])
    test_host_faces.run_refused(case, tmp_path)


# ---- the sidecar ------------------------------------------------------------------------------------------------------
FP = (0x0123456789ABCDEF, 0xFEDCBA9876543210)


def blocks(seed=5):
    rng = np.random.default_rng(seed)
    vol, surf = rng.standard_normal((8, 27 * 8)), rng.standard_normal((8, 54))
    vol[2, 3], vol[7, :5], surf[0, 0] = np.nan, -1.0, -0.0                  # NaN, the "not arrived" mark and -0.0 keep their bits
    return [("volume", vol), ("surface", surf), ("slice_x4", np.zeros((8, 0)))]   # (a rank without faces of a slice: an empty block)


def write(path, **kw):
    from laghos_amd import host_lib
    a = dict(state_fp=FP, ti=3, time=0.0123, R=2, threshold=0.75, sets=blocks())
    a.update(kw)
    host_lib.host_write_records_sidecar(path, a["state_fp"], a["ti"], a["time"], a["R"], a["threshold"], a["sets"])
    return a


def expect(sets):
    return [(t, b.shape[1]) for t, b in sets]


@pytest.mark.parametrize("threshold", [0.75, -0.0, None])
def test_sidecar_round_trip(tmp_path, threshold):
    from laghos_amd import host_lib
    path = str(tmp_path / "cycle_000003.lgr.rec")
    a = write(path, threshold=threshold)
    assert sorted(os.listdir(tmp_path)) == ["cycle_000003.lgr.rec"]         # the .tmp was renamed
    head = open(path, "rb").read(64).split(b"\n")
    assert head[0] == b"LGHREC 1" and head[1].startswith(b"header_bytes ")
    r = host_lib.host_read_records_sidecar(path)
    assert (r["state_fp"], r["ti"], r["R"]) == (FP, 3, 2) and r["time"] == a["time"]
    assert (r["threshold"] is None) == (threshold is None) and (threshold is None or bits([r["threshold"]])[0] == bits([threshold])[0])
    assert [t for t, _ in r["sets"]] == [t for t, _ in a["sets"]]
    for (_, got), (_, want) in zip(r["sets"], a["sets"]):
        assert got.shape == want.shape and np.array_equal(bits(got), bits(want))
    host_lib.host_match_records_sidecar(path, FP, 2, threshold, expect(a["sets"]))
    # the layout: header, the blocks one after the other, two words of trailer
    raw = open(path, "rb").read()
    hb = int(head[1].split()[1])
    words = sum(b.size for _, b in a["sets"])
    assert hb % 64 == 0 and len(raw) == hb + 8 * words + 16
    assert np.array_equal(np.frombuffer(raw[hb:hb + 8 * words], np.uint64), np.concatenate([bits(b).reshape(-1) for _, b in a["sets"]]))
    assert tuple(int(w) for w in np.frombuffer(raw[-16:], np.uint64)) == host_lib.fingerprint_host(np.frombuffer(raw[:-16], np.uint64))


def refused(fn, path, *words):
    from laghos_amd import host_lib
    with pytest.raises(host_lib.RecordsSidecarError) as ex:
        fn()
    msg = str(ex.value)
    assert str(path) in msg and all(w in msg for w in words), msg
    return ex.value.code


def test_sidecar_refusals_each_with_its_own_message(tmp_path):
    from laghos_amd import host_lib
    path = str(tmp_path / "piece.rec")
    a = write(path)
    good = open(path, "rb").read()
    sets = expect(a["sets"])
    read = lambda: host_lib.host_read_records_sidecar(path)
    match = lambda **kw: (lambda: host_lib.host_match_records_sidecar(path, kw.get("fp", FP), kw.get("R", 2), kw.get("thr", 0.75), kw.get("sets", sets)))
    codes = []
    # missing
    codes.append(refused(lambda: host_lib.host_read_records_sidecar(path + ".none"), path + ".none", "missing"))
    # truncated: inside the payload, inside the trailer, inside the header
    for cut in (len(good) // 2, len(good) - 8, 40):
        open(path, "wb").write(good[:cut])
        assert refused(read, path, "truncated") == 4 and refused(match(), path, "truncated") == 4
    codes.append(4)
    # one word too many
    open(path, "wb").write(good + b"\0" * 8)
    codes.append(refused(read, path, "size"))
    # a flipped payload bit, and a flipped trailer bit
    hb = int(good.split(b"\n")[1].split()[1])
    for at in (hb + 8 * 100 + 3, len(good) - 1):
        b = bytearray(good)
        b[at] ^= 0x10
        open(path, "wb").write(bytes(b))
        assert refused(read, path, "trailer") == 6 and refused(match(), path, "trailer") == 6
    codes.append(6)
    # not a sidecar
    open(path, "wb").write(b"LGHCKPT 1\n" + good[10:])
    codes.append(refused(read, path, "magic"))
    # an intact file that is not the one the run continues from
    open(path, "wb").write(good)
    host_lib.host_match_records_sidecar(path, FP, 2, 0.75, sets)
    codes.append(refused(match(fp=(FP[0], FP[1] ^ 1)), path, "state_fp", "another checkpoint"))
    codes.append(refused(match(R=3), path, "-vr", "2", "3"))
    codes.append(refused(match(thr=0.5), path, "threshold", "0.75", "0.5"))
    assert refused(match(thr=None), path, "threshold", "not given") == codes[-1]
    other_count = [sets[0], (sets[1][0], sets[1][1] + 9), sets[2]]
    codes.append(refused(match(sets=other_count), path, "point sets", "surface (54 points)", "surface (63 points)"))
    assert refused(match(sets=sets[:2]), path, "point sets") == codes[-1]
    assert refused(match(sets=[("volume", sets[0][1]), ("slice_y1", 54), sets[2]]), path, "point sets", "slice_y1") == codes[-1]
    assert len(set(codes)) == len(codes) and 0 not in codes                 # every refusal has its own code


def test_writer_refuses_bad_input(tmp_path):
    from laghos_amd import host_lib
    path = str(tmp_path / "no" / "such" / "dir" / "piece.rec")
    with pytest.raises(host_lib.RecordsSidecarError):
        write(path)                                                          # (the sidecar goes beside a piece that exists)
    with pytest.raises(host_lib.RecordsSidecarError):
        write(str(tmp_path / "piece.rec"), sets=[("two words", np.zeros((8, 3)))])
    assert not os.listdir(tmp_path)
