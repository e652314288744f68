"""The host side of checkpoint / restart, without a GPU: lgh_fingerprint_host against a numpy restatement of the function
(tests/fingerprint_ref.py), and the checkpoint file (laghos_amd/host/checkpoint.cpp) through the host probes
laghos_host_write_checkpoint / laghos_host_read_checkpoint: round trip, and every refusal of the reader with its own
message and the caller's arrays untouched."""
import os
import struct

import numpy as np
import pytest

from fingerprint_ref import OFFSETS, combine, data, fp_ref, special_values
from laghos_amd import host_lib

SIZES = (0, 1, 2, 63, 64, 65, 1000)


# ---- the fingerprint --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("n", SIZES)
def test_fingerprint_host_equals_numpy(n, offset):
    x = data(n)
    assert host_lib.fingerprint_host(x, offset) == fp_ref(x, offset)


def test_fingerprint_of_nothing_is_zero():
    assert host_lib.fingerprint_host(np.empty(0), 5) == (0, 0) == fp_ref(np.empty(0), 5)


@pytest.mark.parametrize("offset", OFFSETS)
def test_fingerprint_takes_special_values_as_their_bits(offset):
    x = special_values()
    got = host_lib.fingerprint_host(x, offset)
    assert got == fp_ref(x, offset)
    # -0.0 is not 0.0, a NaN with a payload is not the default NaN
    y = x.copy()
    y[0] = 0.0
    assert host_lib.fingerprint_host(y, offset) != got
    z = x.copy()
    z[3] = z[4]
    assert z.view(np.uint64)[3] != x.view(np.uint64)[3] and host_lib.fingerprint_host(z, offset) != got


def test_fingerprint_of_integers():
    k = np.array([-1, 0, 1, 2 ** 31 - 1, -2 ** 63], dtype=np.int64)
    assert host_lib.fingerprint_host(k, 9) == fp_ref(k, 9)


@pytest.mark.parametrize("offset", OFFSETS)
def test_fingerprint_of_a_concatenation(offset):
    x = data(1000)
    cut = 333
    a, b = host_lib.fingerprint_host(x[:cut], offset), host_lib.fingerprint_host(x[cut:], offset + cut)
    assert combine(a, b) == host_lib.fingerprint_host(x, offset) == fp_ref(x, offset)


def test_fingerprint_is_position_sensitive():
    x = data(1000)
    y = x.copy()
    i, j = 17, 600
    assert x.view(np.uint64)[i] != x.view(np.uint64)[j]
    y[i], y[j] = x[j], x[i]
    a, b = host_lib.fingerprint_host(x), host_lib.fingerprint_host(y)
    assert a[0] != b[0] and a[1] != b[1]
    assert b == fp_ref(y)


def test_fingerprint_host_refuses_bad_arguments():
    from laghos_amd import _lib
    import ctypes
    L = _lib.load()
    out = (ctypes.c_ulonglong * 2)(7, 7)
    x = np.ones(4)
    assert L.lgh_fingerprint_host(ctypes.c_void_p(x.ctypes.data), -1, 0, out) == 1      # LGH_ERR_ARG
    assert L.lgh_fingerprint_host(None, 3, 0, out) == 1
    assert tuple(out) == (7, 7)
    assert L.lgh_fingerprint_host(None, 0, 0, out) == 0 and tuple(out) == (0, 0)


# ---- the file ---------------------------------------------------------------------------------------------------------
def bits(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def make_header():
    return dict(dim=3, problem=1, order_v=3, order_e=2, Q1D=8, NE=64, global_NE=128, N=2197, nranks=2, rank=1, pgrid0=2, pgrid1=1,
                pgrid2=1, ode_solver=7, cg_max_iter=301, ti=40, steps=43, repeats=3, checks=1, checks_ok=1,
                cfl=0.1 + 0.2, cg_tol=1e-8 / 3.0, t=np.nextafter(0.3, 1.0), dt=5e-324, energy_init=-0.0,
                setup_fp=(0xFEDCBA9876543210, 0x0123456789ABCDEF))


@pytest.fixture(scope="module")
def written(tmp_path_factory):
    """one checkpoint written through the host probe: (path, header, S, pv_times, pv_cycles, the file's bytes)"""
    d = tmp_path_factory.mktemp("ckpt")
    path = str(d / "deep" / "er" / "run_restart" / "cycle_000040.lgr.1")
    S = data(1237, seed=3)
    t = np.array([0.0, 0.125, np.nextafter(0.25, 1.0)])
    c = np.array([0, 20, 40], dtype=np.int64)
    h = make_header()
    host_lib.host_write_checkpoint(path, h, S, t, c)
    return path, h, S, t, c, open(path, "rb").read()


def read_into_fresh(path, n=2000, npv=8):
    S, t, c = np.full(n, 123.0), np.full(npv, 456.0), np.full(npv, 789, dtype=np.int64)
    return host_lib.host_read_checkpoint(path, S, t, c), S, t, c


def test_round_trip(written):
    path, h, S, t, c, raw = written
    assert not os.path.exists(path + ".tmp") and os.listdir(os.path.dirname(path)) == [os.path.basename(path)]
    got, S2, t2, c2 = read_into_fresh(path)
    for k, v in h.items():
        if isinstance(v, float):
            assert bits(got[k]) == bits(v), k                 # the bits of every double, -0.0 and the denormal included
        else:
            assert got[k] == v, k
    assert got["state_words"] == S.size and got["paraview_dumps"] == 3
    assert got["state_fp"] == fp_ref(S)
    assert np.array_equal(S2[:S.size].view(np.uint64), S.view(np.uint64)) and np.all(S2[S.size:] == 123.0)
    assert np.array_equal(t2[:3].view(np.uint64), t.view(np.uint64)) and np.array_equal(c2[:3], c)
    # the layout of DESIGN.md 7c: padded ASCII header, raw payload, trailer = fingerprint of everything before it
    hb = got["header_bytes"]
    assert hb % 4096 == 0 and len(raw) == hb + 8 * (S.size + 2 * 3) + 16
    head = raw[:hb].decode("ascii")
    lines = head.split("\n")
    assert lines[0] == "LGHCKPT 1" and lines[1] == f"header_bytes {hb}" and "end" in lines
    assert set(head[head.index("\nend\n") + 5:]) == {"\n"}
    assert f"t {bits(h['t']):016X} #" in head and f"state_words {S.size}\n" in head
    body = np.frombuffer(raw[:-16], dtype=np.uint64)
    assert fp_ref(body) == struct.unpack("<2Q", raw[-16:])
    assert np.array_equal(np.frombuffer(raw[hb:hb + 8 * S.size], dtype=np.uint64), S.view(np.uint64))


def test_an_empty_checkpoint_round_trips(tmp_path):
    path = str(tmp_path / "empty.lgr")
    host_lib.host_write_checkpoint(path, make_header(), np.empty(0))
    got, S, t, c = read_into_fresh(path)
    assert got["state_words"] == 0 and got["paraview_dumps"] == 0 and got["state_fp"] == (0, 0) and np.all(S == 123.0)


def with_trailer(body):
    return body + struct.pack("<2Q", *fp_ref(np.frombuffer(body, dtype=np.uint64)))


def flip(raw, byte, bit=0):
    b = bytearray(raw)
    b[byte] ^= 1 << bit
    return bytes(b)


def damaged_files(raw):
    """name -> (bytes, error code of checkpoint.hpp, words the message must hold)"""
    head_end = raw.index(b"\nend\n")
    hb = int(raw.split(b"\n")[1].split()[1])
    t_at = raw.index(b"\nt ") + 3 + 15                           # the last hex digit of t
    sw = raw.index(b"state_words ")
    smaller = raw[:sw] + b"state_words 1236" + raw[sw + len(b"state_words 1237"):]
    return {
        "wrong magic": (b"LGHCKPX" + raw[7:], 2, ["magic"]),
        "version 2": (raw[:8] + b"2" + raw[9:], 3, ["version", "2"]),
        "bit in the header": (flip(raw, t_at), 7, ["trailer", "header"]),
        "bit in the payload": (flip(raw, hb + 8 * 100 + 3, 5), 7, ["trailer", "state"]),
        "bit in the trailer": (flip(raw, len(raw) - 1, 7), 7, ["trailer"]),
        "cut in the payload": (raw[:hb + 8 * 500 + 3], 5, ["truncated"]),
        "cut inside the header": (raw[:head_end - 40], 4, ["header_bytes"]),
        "state_words against the size": (smaller, 6, ["size", "state_words"]),
        # only state_fp can catch this one: the payload altered and the trailer made anew
        "payload altered, trailer recomputed": (with_trailer(flip(raw, hb + 8 * 7, 1)[:-16]), 8, ["state_fp"]),
    }


def test_refusals(written, tmp_path):
    path, h, S, t, c, raw = written
    messages = {}
    for name, (content, code, words) in damaged_files(raw).items():
        p = str(tmp_path / (name.replace(" ", "_").replace(",", "") + ".lgr"))
        with open(p, "wb") as f:
            f.write(content)
        with pytest.raises(host_lib.CheckpointError) as ei:
            S2, t2, c2 = np.full(2000, 123.0), np.full(8, 456.0), np.full(8, 789, dtype=np.int64)
            host_lib.host_read_checkpoint(p, S2, t2, c2)
        msg = str(ei.value)
        print(f"{name}: [{ei.value.code}] {msg}")
        assert ei.value.code == code, (name, msg)
        assert p in msg and all(w in msg for w in words), (name, msg)
        assert np.all(S2 == 123.0) and np.all(t2 == 456.0) and np.all(c2 == 789), name   # nothing of the caller's was touched
        messages[name] = msg.replace(p, "")
    # every refusal has its own message (numbers taken out: two trailer failures differ in more than their hex digits)
    import re
    shapes = {n: re.sub(r"[0-9A-F]{16,}|\d+", "#", m) for n, m in messages.items()}
    assert len(set(shapes.values())) >= len(shapes) - 1, shapes   # (a bit in the header and one in the trailer read alike)
    assert shapes["bit in the payload"] != shapes["bit in the header"]


def test_missing_file_and_small_arrays(written, tmp_path):
    path = written[0]
    with pytest.raises(host_lib.CheckpointError) as ei:
        read_into_fresh(str(tmp_path / "nothing.lgr"))
    assert ei.value.code == 1 and "cannot open" in str(ei.value)
    with pytest.raises(host_lib.CheckpointError) as ei:
        read_into_fresh(path, n=100)
    assert ei.value.code == 9


def test_write_leaves_no_tmp_and_replaces_atomically(tmp_path):
    path = str(tmp_path / "a.lgr")
    for k in range(2):
        host_lib.host_write_checkpoint(path, dict(make_header(), ti=k), data(10, seed=k))
        assert sorted(os.listdir(tmp_path)) == ["a.lgr"]
        assert read_into_fresh(path)[0]["ti"] == k
