"""Host side of two items of the specialised training loop — no GPU needed.

SPEC_QUADS (specialize.cpp BSVI_SPEC_QUADS; spec_prelude.h): the table values one Normal record reads — location offset, scale,
1 / scale, log scale — are one 16-byte group of LDS, four observations another, each read with one 16-byte load.  The generated
map, what the generator emits with the switch off, and what the compiler makes of it.

SPEC_OPT_LITERAL (spec_main.h; specialize.cpp opt_literal): the owners' epilogue of variant 6 compiled for one optimizer.  Which
code object a launch takes, as a function of the configuration and BSVI_SPEC_OPT_LITERAL, and what the compiler makes of variant 6
under each literal.

What the kernels compute is compared bit for bit with the switches at 0 on the GPU (tests/test_gpu_spec_quads.py)."""
import collections
import os
import re
import subprocess

import pytest

from brancher_amd import native
from test_spec_trim_cpu import LLVM, code_object, headline, programs


def counts(src, tmp_path, monkeypatch, tag):
    """code_object's counts and metadata (with the static LDS size), and the opcode histogram of the same code object"""
    totals, meta = code_object(src, tmp_path, monkeypatch, tag)
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", str(tmp_path / ("%s.co" % tag))], capture_output=True, text=True).stdout
    meta = dict(meta, lds_bytes=int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", notes).group(1)))
    text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", str(tmp_path / ("%s.co" % tag))], capture_output=True, text=True).stdout
    ops = collections.Counter(line.split()[0] for line in text.splitlines() if line.startswith("\t"))
    assert sum(ops.values()) == totals["total"]
    return totals, meta, ops


def test_literal_objects_are_shorter_and_need_no_more_registers(tmp_path, monkeypatch):
    """variant 6 of README AR T = 20 behind `#define SPEC_OPT_LITERAL n`: both literals compile, each to fewer instructions than
    the generic object and to no more vector registers; the SGD object carries none of the other kinds' divisions (Adam's are
    what the Adam object has beyond the SGD object's: both hold the rest of the kernel) and no double-precision bias factors"""
    assert os.path.exists(os.path.join(LLVM, "llvm-objdump")), "llvm-objdump of the ROCm toolchain disassembles the code objects"
    src = native.specialised_source(headline(), 6)
    assert "SPEC_OPT_LITERAL" not in src                  # (the launch puts the define in front: not a property of the variant)
    made = {n: counts("#define SPEC_OPT_LITERAL %d\n" % n + src, tmp_path, monkeypatch, "literal%d" % n) for n in (0, 1, 2)}
    plain = counts(src, tmp_path, monkeypatch, "plain")
    div = lambda n: made[n][2]["v_div_scale_f32"]
    f64 = lambda n: sum(k for op, k in made[n][2].items() if op.endswith("_f64"))
    for n in (0, 1, 2):
        print("literal %d:" % n, made[n][0], made[n][1], "v_div_scale_f32", div(n), "f64 instructions", f64(n))
    assert made[0][0] == plain[0] and made[0][1] == plain[1]              # 0 is the generic object
    for n in (1, 2):
        assert made[n][1]["vgpr_spill_count"] == 0 and made[n][1]["private_segment_fixed_size"] == 0, made[n][1]
        assert made[n][1]["vgpr_count"] <= made[0][1]["vgpr_count"] <= 228, (made[n][1], made[0][1])
        assert made[n][0]["total"] < made[0][0]["total"], (n, made[n][0], made[0][0])
    adams = div(2) - div(1)
    assert adams > 0 and div(1) <= div(0) - adams, (div(0), div(1), div(2))
    assert f64(1) < f64(2) < f64(0)


def test_a_literal_beyond_the_two_does_not_compile(monkeypatch):
    src = native.specialised_source(headline(), 6)
    monkeypatch.delenv("BSVI_JIT_DUMP", raising=False)
    with pytest.raises(Exception):
        native.jit_compile("#define SPEC_OPT_LITERAL 3\n" + src)


def test_kernels_without_the_lean_owners_loop_ignore_the_define(tmp_path, monkeypatch):
    """variant 0 (no owners' wave): the define changes nothing"""
    src = native.specialised_source(headline(), 0)
    a = code_object(src, tmp_path, monkeypatch, "v0")
    b = code_object("#define SPEC_OPT_LITERAL 1\n" + src, tmp_path, monkeypatch, "v0literal")
    assert a == b


CONFIGURATIONS = [
    # optimizer, options, literal
    ("SGD", dict(lr=1e-3), 1),
    ("SGD", dict(lr=0.5), 1),                                            # (the learning rate stays data)
    ("SGD", dict(lr=1e-3, momentum=0.9), 0),
    ("SGD", dict(lr=1e-3, momentum=0.9, nesterov=True), 0),
    ("SGD", dict(lr=1e-3, weight_decay=1e-2), 0),
    ("SGD", dict(lr=1e-3, maximize=True), 0),
    ("Adam", dict(lr=1e-2), 2),
    ("Adam", dict(lr=1e-3, betas=(0.8, 0.95), eps=1e-6), 2),              # (betas and eps stay data)
    ("Adam", dict(lr=1e-2, amsgrad=True), 0),
    ("Adam", dict(lr=1e-2, weight_decay=1e-2), 0),
    ("Adam", dict(lr=1e-2, maximize=True), 0),
    ("AdamW", dict(lr=1e-2), 0),
    ("RMSprop", dict(lr=1e-3), 0),
    ("Adagrad", dict(lr=1e-2), 0),
    ("Adamax", dict(lr=5e-3), 0),
]


@pytest.mark.parametrize("optimizer,kw,literal", CONFIGURATIONS)
def test_the_launch_plan_names_the_object(optimizer, kw, literal, monkeypatch):
    """bsvi_spec_opt_literal: what a launch of the owners' loop with this configuration takes; BSVI_SPEC_OPT_LITERAL=0, read at
    every call, names the generic object always"""
    lib = native.load()
    cfg = native.make_opt_cfg(optimizer, **kw)
    monkeypatch.delenv("BSVI_SPEC_OPT_LITERAL", raising=False)
    assert lib.bsvi_spec_opt_literal(cfg) == literal
    monkeypatch.setenv("BSVI_SPEC_OPT_LITERAL", "0")
    assert lib.bsvi_spec_opt_literal(cfg) == 0
    monkeypatch.setenv("BSVI_SPEC_OPT_LITERAL", "1")
    assert lib.bsvi_spec_opt_literal(cfg) == literal
    assert lib.bsvi_spec_opt_literal(None) == 0


# ---- SPEC_QUADS ------------------------------------------------------------------------------------------------------------------
NO_QUADS = "#define SPEC_DEBUG_NO_QUADS 1\n"
QUAD_LINE = re.compile(r"^(// SPEC_QUADS: .*|#define SPEC_QUADS_MAP 1|#define SPEC_Q_GROUPS \d+|// per entry, in float offsets: .*|#define SPEC_Q_HOMES .*"
                       r"|#define SPEC_QV_[URL]_\d+ .*|    SPEC_[QO](LOAD|VAR)\(\d+\);)$")


def without_quads(src):
    """the generated source with the map's defines and the groups' loads taken out"""
    return "".join(line + "\n" for line in src.split("\n")[:-1] if not QUAD_LINE.match(line))


def pad4(n):
    return (n + 3) // 4 * 4


def table_map(src):
    """the generated map: (groups, n_uniform, n_obs, {(entry, 'U' | 'R' | 'L'): home in floats}, homes of SPEC_Q_HOMES)"""
    n_uniform = int(re.search(r"#define SPEC_N_UNIFORM (\d+)", src).group(1))
    n_obs = int(re.search(r"#define SPEC_N_OBS (\d+)", src).group(1))
    groups = int(re.search(r"#define SPEC_Q_GROUPS (\d+)", src).group(1))
    obs0 = pad4(3 * n_uniform)
    homes = {}
    for which, k, kind, a, b in re.findall(r"#define SPEC_QV_([URL])_(\d+) SPEC_Q([GMO])\((\d+)(?:, ([xyzw]))?\)", src):
        key = (int(k), which)
        assert key not in homes, key                                     # one home per value
        if kind == "G":
            assert int(a) < groups
            homes[key] = 4 * int(a) + "xyzw".index(b)
        elif kind == "O":
            homes[key] = obs0 + 4 * int(a) + "xyzw".index(b)
        else:
            homes[key] = int(a)
    packed = [int(x, 16) for x in re.findall(r"0x([0-9a-f]{8})u", re.search(r"#define SPEC_Q_HOMES \{(.*)\}", src).group(1))]
    return groups, n_uniform, n_obs, homes, packed


def body_reads(src):
    """every (entry, which) the body's text reads, SPEC_SAME resolved"""
    body = src.split("void spec_body")[1].split("#include \"spec_main.h\"")[0]
    reads = set()
    for which, k0, k in re.findall(r"SPEC_U([RL]?)\((?:SPEC_SAME\(\d+, (\d+)\)|(\d+))\)", body):
        reads.add((int(k0 or k), which or "U"))
    return reads


def check_map(src):
    groups, n_uniform, n_obs, homes, packed = table_map(src)
    obs0 = pad4(3 * n_uniform)
    # every value of the table and every observation has exactly one home; no two homes overlap
    assert sorted(homes) == sorted([(k, w) for k in range(n_uniform) for w in "ULR"] + [(n_uniform + i, "U") for i in range(n_obs)])
    assert len(set(homes.values())) == len(homes)
    # every value the body reads is one of them
    reads = body_reads(src)
    assert reads and reads <= set(homes), sorted(reads - set(homes))[:5]
    # the table's values fill [0, 3 n_uniform) — the groups first, 16-byte aligned — and the observations follow, contiguous, aligned
    assert sorted(h for (k, w), h in homes.items() if k < n_uniform) == list(range(3 * n_uniform))
    assert obs0 % 4 == 0 and [homes[(n_uniform + i, "U")] for i in range(n_obs)] == list(range(obs0, obs0 + n_obs))
    grouped = collections.defaultdict(dict)
    for (k, w), h in homes.items():
        if h < 4 * groups:
            grouped[h // 4][h % 4] = (k, w)
    assert sorted(grouped) == list(range(groups))
    for g, members in grouped.items():
        # {U[c], U[s], 1/U[s], log U[s]}
        (c, wc), (s, ws), (r, wr), (l, wl) = (members[i] for i in range(4))
        assert (wc, ws, wr, wl) == ("U", "U", "R", "L") and s == r == l and c != s, (g, members)
    # 1 / U and log U of an entry are neighbours, and SPEC_Q_HOMES (what the writers use) says the same as the per-value defines
    assert len(packed) == n_uniform
    for k in range(n_uniform):
        assert homes[(k, "L")] == homes[(k, "R")] + 1
        assert packed[k] == homes[(k, "U")] | (homes[(k, "R")] << 16), k
    return groups, n_uniform, n_obs


def test_headline_map_and_reads(tmp_path, monkeypatch):
    """variant 6 of README AR T = 20: the 21 sampled nodes' values are 21 groups; against the same source with
    SPEC_DEBUG_NO_QUADS at least 20 fewer LDS reads, fewer instructions, at most 228 registers and no spill; the static LDS of
    each code object is what its layout says"""
    src = native.specialised_source(headline(), 6)
    groups, n_uniform, n_obs = check_map(src)
    assert (groups, n_uniform, n_obs) == (21, 65, 20)
    assert src.count("SPEC_QLOAD(") == 21 and src.count("SPEC_OLOAD(") == 5
    on, on_meta, _ = counts(src, tmp_path, monkeypatch, "quads")
    off, off_meta, _ = counts(NO_QUADS + src, tmp_path, monkeypatch, "noquads")
    print("SPEC_DEBUG_NO_QUADS:", off, off_meta)
    print("default:            ", on, on_meta)
    assert off["ds_read"] - on["ds_read"] >= 20, (on, off)
    assert on["total"] < off["total"], (on, off)
    assert on_meta["vgpr_count"] <= 228 and on_meta["vgpr_spill_count"] == 0 and on_meta["private_segment_fixed_size"] == 0, on_meta
    compact = pad4(n_uniform + n_obs) + 2 * pad4(n_uniform)
    grouped = pad4(pad4(3 * n_uniform) + n_obs)
    assert grouped <= compact
    assert off_meta["lds_bytes"] - on_meta["lds_bytes"] == 4 * (compact - grouped), (on_meta, off_meta)
    # the shared constants' switch takes the layout with it (tests/test_spec_trim_cpu.py compares that build with BSVI_SPEC_TRIM=0)
    shared, shared_meta, _ = counts("#define SPEC_DEBUG_NO_SHARED_CONST 1\n" + src, tmp_path, monkeypatch, "noshared")
    assert shared_meta["lds_bytes"] == off_meta["lds_bytes"] and shared["ds_read"] >= off["ds_read"]


def test_switch_off_generates_every_source_without_the_map(monkeypatch):
    """BSVI_SPEC_QUADS=0, read when the program is created: every variant of the four programs is the default source with the
    map's defines and the groups' loads taken out — and the default source itself where no record forms a group"""
    monkeypatch.setenv("BSVI_SPEC_LEAN_CHAIN", "1")      # (variant 7 exists only when this is set)
    default = {name: [native.specialised_source(p, v) or "" for v in range(8)] for name, p in programs().items()}
    monkeypatch.setenv("BSVI_SPEC_QUADS", "0")
    off = {name: [native.specialised_source(p, v) or "" for v in range(8)] for name, p in programs().items()}
    for name in default:
        for v in range(8):
            assert "SPEC_Q" not in off[name][v] and "SPEC_OLOAD" not in off[name][v], (name, v)
            assert without_quads(default[name][v]) == off[name][v], (name, v)
            if "SPEC_QUADS_MAP" not in default[name][v]:
                assert default[name][v] == off[name][v]
    assert all("SPEC_QUADS_MAP" in s for s in default["readme_ar_T20"] if s)
    assert not any("SPEC_QUADS_MAP" in s for s in default["beta_binomial"])      # (no Normal record: nothing to group)


@pytest.mark.parametrize("name,variant", [("two_entry", 0), ("two_entry", 6), ("readme_ar_T200", 0), ("readme_ar_T200", 2), ("beta_binomial", 0)])
def test_other_programs_get_a_layout_and_compile_without_spills(name, variant, tmp_path, monkeypatch):
    """a parameter with two entries (the owners' rows carry two homes), the T = 200 program (DPP row sums; the groups are loaded
    again in the reverse sweep), beta-binomial (no group: the compact layout)"""
    src = native.specialised_source(programs()[name], variant)
    if name == "beta_binomial":
        assert "SPEC_QUADS_MAP" not in src
    else:
        groups, n_uniform, n_obs = check_map(src)
        print(name, variant, "groups", groups, "of", n_uniform, "entries,", n_obs, "observations")
        assert groups > 0
    totals, meta, _ = counts(src, tmp_path, monkeypatch, "%s%d" % (name, variant))
    print(totals, meta)
    assert meta["vgpr_spill_count"] == 0, meta
    # (beta-binomial calls its generic distributions out of line: 16 bytes of stack, in the same source as with the switch off)
    assert meta["private_segment_fixed_size"] == (16 if name == "beta_binomial" else 0), meta
