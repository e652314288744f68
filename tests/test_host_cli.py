"""The command line of the `laghos` executable where it refuses: every refusal of the option parser and of the checks that
need the mesh's dimension and zone grid happens before the first GPU call, so the cases run without a GPU.  Each case runs the
executable once and holds it to exit status 1, the complete stdout (empty, but for the line a 1D mesh prints when it switches
-pa to -fa before its refusal) and the complete stderr, and nothing created under a fresh -k base.

The expected texts are what the driver printed before its options moved into a file of their own.  The last group are command
lines with a quirk that must NOT be refused where the quirk sits: a refusal further along the same line shows that the parser
went past it."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "laghos_amd", "laghos")

TO_FA = "Laghos does not support PA in 1D. Switching to FA.\n"
UNKNOWN_FIELD = " (div_v, vorticity, grad_v, detj, sound_speed or all)"
EMPTY_LIST = "-pv-fields needs a list of div_v, vorticity, grad_v, detj, sound_speed, or all: the list is empty"
NO_FACES_1D = ": zone faces are dumped in 2D and 3D, this mesh is 1D (its -paraview dump is small already)"
EIGHT_SLICES = sum((["-pv-slice", "x", str(k)] for k in range(8)), [])

# (arguments, stderr without its newline); the message carries `laghos: ` unless the case is in NO_PREFIX below
PARSER = [
    # a value is missing: one option of each shape
    (["-ms"], "missing value for -ms"),
    (["-tf"], "missing value for -tf"),
    (["-m"], "missing value for -m"),
    (["-ckpt"], "missing value for -ckpt"),
    (["-ckpt-keep"], "missing value for -ckpt-keep"),
    (["-hist"], "missing value for -hist"),
    (["-prof"], "missing value for -prof"),
    (["-prof-axis"], "missing value for -prof-axis"),
    (["-prof-bins"], "missing value for -prof-bins"),
    (["-prof-range"], "missing value for -prof-range"),
    (["-prof-range", "1"], "missing value for 1"),
    (["-map"], "missing value for -map"),
    (["-restart"], "missing value for -restart"),
    (["-vr"], "missing value for -vr"),
    (["-pv-fields"], "missing value for -pv-fields"),
    (["-pv-slice"], "missing value for -pv-slice AXIS K"),
    (["-pv-slice", "x"], "missing value for -pv-slice AXIS K"),
    (["--paraview-slice", "x"], "missing value for --paraview-slice AXIS K"),
    (["-renumber"], "missing value for -renumber"),
    (["-k"], "missing value for -k"),
    (["-d"], "missing value for -d"),
    # a value is refused
    (["-ckpt", "0"], "-ckpt / --checkpoint-steps must be at least 1, got 0"),
    (["--checkpoint-steps", "abc"], "-ckpt / --checkpoint-steps must be at least 1, got abc"),
    (["-ckpt", "3", "-ckpt", "0"], "-ckpt / --checkpoint-steps must be at least 1, got 0"),
    (["-ckpt", "0", "-ckpt", "3"], "-ckpt / --checkpoint-steps must be at least 1, got 0"),
    (["-ckpt-keep", "-1"], "-ckpt-keep / --checkpoint-keep must be 0 (keep all) or more, got -1"),
    (["-hist", "0"], "-hist / --history-steps must be at least 1, got 0"),
    (["-prof", "-3"], "-prof / --profile-steps must be at least 1, got -3"),
    (["-map", "0"], "-map / --map-steps must be at least 1, got 0"),
    (["-prof-axis", "w"], "-prof-axis must be x, y, z or r, got w"),
    (["-prof-bins", "0"], "-prof-bins must be between 1 and 4096, got 0"),
    (["-prof-bins", "4097"], "-prof-bins must be between 1 and 4096, got 4097"),
    (["-prof-range", "a", "1"], "-prof-range needs two numbers, got a"),
    (["-prof-range", "0", "1x"], "-prof-range needs two numbers, got 1x"),
    (["-prof-range", "2", "1"], "-prof-range LO HI needs finite LO < HI"),
    (["-prof-range", "0", "inf"], "-prof-range LO HI needs finite LO < HI"),
    (["-prof-range", "0", "1", "-prof-range", "1", "0"], "-prof-range LO HI needs finite LO < HI"),
    (["-prof-origin", "inf"], "-prof-origin needs finite coordinates"),
    (["-prof-origin"], "-prof-origin needs one to three numbers"),
    (["-prof-origin", "x"], "-prof-origin needs one to three numbers"),
    (["-map-cells", "0"], "-map-cells needs counts between 1 and 1048576, got 0"),
    (["-map-cells", "4", "1048577"], "-map-cells needs counts between 1 and 1048576, got 1048577"),
    (["-map-cells"], "-map-cells needs one to three counts"),
    (["-map-cells", "-bogus"], "-map-cells needs one to three counts"),
    (["-map-box"], "-map-box needs a pair LO HI per axis, got 0 numbers"),
    (["-map-box", "0"], "-map-box needs a pair LO HI per axis, got 1 numbers"),
    (["-map-box", "0", "1", "2"], "-map-box needs a pair LO HI per axis, got 3 numbers"),
    (["-map-box", "2", "1"], "-map-box needs finite LO < HI on every axis"),
    (["-map-box", "0", "1", "0", "nan"], "-map-box needs finite LO < HI on every axis"),
    (["-restart", ""], "-restart needs a checkpoint stem or the word latest"),
    (["-paraview", "-pv-fields", "foo"], "-pv-fields: unknown field foo" + UNKNOWN_FIELD),
    (["-paraview", "-pv-fields", "div_v,,curl"], "-pv-fields: unknown field curl" + UNKNOWN_FIELD),
    (["-paraview", "-pv-fields", ","], EMPTY_LIST),
    (["-paraview", "-pv-fields", ""], EMPTY_LIST),
    (["-pv-slice", "w", "1"], "-pv-slice AXIS K: the axis must be x, y or z, got w"),
    (["-pv-slice", "x", "-1"], "-pv-slice x K: K must be a node plane 0 <= K <= n of the zone grid, got -1"),
    (["-pv-slice", "x", "1.5"], "-pv-slice x K: K must be a node plane 0 <= K <= n of the zone grid, got 1.5"),
    (["-pv-slice", "x", "3", "-pv-slice", "x", "3"], "-pv-slice x 3 is given twice"),
    (EIGHT_SLICES + ["-pv-slice", "y", "0"], "-pv-slice y 0: at most 8 slices, this is the ninth"),
    (["-bogus"], "unsupported option: -bogus"),
    # what the parser checks once the whole line is read
    (["-vr", "9"], "-vr / --vis-refine must be between 1 and 8, got 9"),
    (["-vr", "abc"], "-vr / --vis-refine must be between 1 and 8, got 0"),
    (["-paraview", "-vr", "0"], "-vr / --vis-refine must be between 1 and 8, got 0"),
    (["-paraview", "-ok", "9"], "-vr / --vis-refine must be between 1 and 8, got 9"),
    (["-pv-fields", "div_v"], "-pv-fields adds fields to the -paraview dumps: it needs -paraview"),
    (["-paraview", "-no-paraview", "-pv-fields", "all"], "-pv-fields adds fields to the -paraview dumps: it needs -paraview"),
    (["-map-cells", "4"], "-map-cells describes the -map files: it needs -map"),
    (["-map-box", "0", "1"], "-map-box describes the -map files: it needs -map"),
    (["-map-cells", "4", "-map-box", "0", "1"], "-map-cells describes the -map files: it needs -map"),
]

# between the mesh and the discretisation; a third entry is the stdout (a 1D mesh under the default -pa says that it switches)
MESH = [
    (["-err", "-p", "0"], "Can only compare problem 1 (Sedov) against the exact solution"),
    (["-err", "-m", "data/square01_quad.mesh"], "check: mesh_file"),
    (["-dim", "1", "-paraview", "-pv-fields", "vorticity"], "-pv-fields vorticity: there is no vorticity in 1D", TO_FA),
    (["-dim", "1", "-q", "-paraview", "-pv-fields", "all,vorticity"], "-pv-fields vorticity: there is no vorticity in 1D"),
    (["-dim", "1", "-pv-surface"], "-pv-surface" + NO_FACES_1D, TO_FA),
    (["-dim", "1", "-pv-slice", "x", "1"], "-pv-slice" + NO_FACES_1D, TO_FA),
    (["-m", "data/segment01.mesh", "-fa", "-pv-surface", "-pv-slice", "x", "1"], "-pv-surface" + NO_FACES_1D),
    (["-dim", "1", "-paraview", "-pv-fields", "all", "-pv-slice", "x", "1"], "-pv-slice" + NO_FACES_1D, TO_FA),    # (`all` drops vorticity in 1D)
    (["-dim", "2", "-pv-slice", "z", "1"], "-pv-slice z 1: the mesh has 2 dimensions, there is no z axis"),
    (["-pv-slice", "x", "9"], "-pv-slice x 9: K is out of range, the zone grid has node planes 0..8 along x"),
    (["-dim", "2", "-rs", "1", "-pv-slice", "y", "4", "-pv-slice", "y", "5"],
     "-pv-slice y 5: K is out of range, the zone grid has node planes 0..4 along y"),
    (["-prof", "2", "-prof-axis", "z", "-dim", "2"], "-prof-axis z needs a mesh of 3 dimensions, this one has 2"),
    (["-prof", "2", "-prof-axis", "y", "-dim", "1"], "-prof-axis y needs a mesh of 2 dimensions, this one has 1", TO_FA),
    (["-map", "2", "-map-cells", "4", "4", "-dim", "3"], "-map-cells has 2 counts, the mesh has 3 dimensions"),
    (["-map", "2", "-map-box", "0", "1", "0", "1", "-dim", "3"], "-map-box has 4 numbers, a mesh of 3 dimensions needs 6"),
    (["-map", "2", "-map-cells", "1024", "1024", "2"], "-map-cells asks for 2097152 cells, at most 1048576 fit"),
    (["-map", "2", "-dim", "2", "-map-cells", "1024", "1025"], "-map-cells asks for 1049600 cells, at most 1048576 fit"),
    (["-fa"], "only the partial-assembly path (-pa) is implemented"),
    (["-fa", "-dim", "2"], "only the partial-assembly path (-pa) is implemented"),
    (["LGH_FORCE_MULTI=1", "-dim", "1"], "LGH_FORCE_MULTI=1 drives the multi-rank path, which 1D does not have", TO_FA),
    (["LGH_FORCE_MULTI=1", "-dim", "1", "-fa"], "LGH_FORCE_MULTI=1 drives the multi-rank path, which 1D does not have"),
    # what the mesh and the discretisation themselves refuse comes out of the same place
    (["-m", "nosuch.mesh"], "mesh 'nosuch.mesh' is not one of the structured meshes this harness supports (segment01, square01_quad, "
                            "cube01_hex, box01_hex, rectangle01_quad, square_gresho, rt2D)"),
    (["-dim", "1", "-p", "3"], "problem 3 is not defined in 1D: only problems 1 (Sedov) and 2 (Sod) are", TO_FA),
]
NO_PREFIX = ("Can only compare problem 1 (Sedov) against the exact solution", "check: mesh_file")

# accepted where the quirk sits: the message is that of what follows it
QUIRKS = [
    (["-prof-origin", "1", "2", "-prof", "3", "-bogus"], "unsupported option: -bogus"),           # the list ends at the first non-number
    (["-prof-origin", "1", "2x", "-bogus"], "unsupported option: 2x"),                            # ... a complete number, that is
    (["-prof-origin", "1", "2", "3", "4"], "unsupported option: 4"),                              # ... or when it is full
    (["-map-cells", "1", "2", "3", "4"], "unsupported option: 4"),
    (["-map", "1", "-map-box", "0", "1", "1e", "-bogus"], "unsupported option: 1e"),
    (["-map-box", "0", "1", "0", "1", "0", "1", "7", "-bogus"], "unsupported option: 7"),
    (["-map", "2", "-map-cells", "4", "-map-cells", "4", "4", "4", "-bogus"], "unsupported option: -bogus"),
    (["-map", "2", "-map-cells", "4", "4", "4", "-map-cells", "4", "-dim", "3"], "-map-cells has 1 counts, the mesh has 3 dimensions"),   # the count restarts
    (["-ms", "abc", "-bogus"], "unsupported option: -bogus"),                                     # atoi: 0
    (["-d", "-bogus", "-bogus2"], "unsupported option: -bogus2"),                                 # -d swallows its value
    (["-hist", "3", "-hist", "2", "-bogus"], "unsupported option: -bogus"),
    (["-vr", "9", "-vr", "2", "-bogus"], "unsupported option: -bogus"),                           # -vr is checked at the end of the line
    (["-no-vis", "-no-visit", "-no-print", "--no-visualization", "-bogus"], "unsupported option: -bogus"),
    (["-pv-slice", "x", "3", "-pv-slice", "y", "3", "-bogus"], "unsupported option: -bogus"),
    (["-paraview", "-pv-fields", "all", "-pv-fields", "detj,", "-bogus"], "unsupported option: -bogus"),
    (["-pv-surface", "-pv-fields", "all", "-bogus"], "unsupported option: -bogus"),               # a face dump will do for -pv-fields
]


def case_id(case):
    return " ".join(a if a else "''" for a in case[0])


def refused(case, tmp_path):
    args, message = case[0], case[1]
    stdout = case[2] if len(case) > 2 else ""
    env = {k: v for k, v in os.environ.items() if k != "LGH_FORCE_MULTI"}
    while args and "=" in args[0] and not args[0].startswith("-"):
        name, value = args[0].split("=", 1)
        env[name] = value
        args = args[1:]
    base = tmp_path / "base"
    base.mkdir()
    p = subprocess.run([EXE, "-k", str(base / "out" / "run")] + args, capture_output=True, text=True, timeout=60, cwd=ROOT, env=env)
    prefix = "" if message in NO_PREFIX else "laghos: "
    assert (p.returncode, p.stdout, p.stderr) == (1, stdout, prefix + message + "\n")
    assert os.listdir(base) == []


@pytest.mark.parametrize("case", PARSER, ids=case_id)
def test_the_parser_refuses(case, tmp_path):
    refused(case, tmp_path)


@pytest.mark.parametrize("case", MESH, ids=case_id)
def test_the_mesh_dependent_checks_refuse(case, tmp_path):
    refused(case, tmp_path)


@pytest.mark.parametrize("case", QUIRKS, ids=case_id)
def test_quirks_are_accepted_where_they_sit(case, tmp_path):
    refused(case, tmp_path)
