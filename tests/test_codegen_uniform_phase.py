"""CPU: the re-encoded loop bodies of the plain search kernels.

The build puts csrc/phase_rewrite between the device compile of kernels_plain.hip and the
assembler: in the per-nonce loop of every k_scan<J,0,false,0> the Makefile lists (UNIFORM_J),
each VALU instruction is 8 bytes and sits at the code phase of the pin, 4 mod 8, and nothing
is added, removed or reordered.  This reads the product's code object and checks exactly
that, against the compiler's own output for the same source; then the rewriter's functions on
a hand-written fixture (tests/golden/phase_rewrite/), and stand-alone under ASan + UBSan.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "bitcoin-miner_amd")
LLVM = "/opt/rocm/lib/llvm/bin"
FIX = os.path.join(ROOT, "tests", "golden", "phase_rewrite")
INSN = re.compile(r"\s+([vs]_\S+|global_\S+|scratch_\S+|ds_\S+|buffer_\S+|flat_\S+)\s(.*)//\s*([0-9A-Fa-f]+):((?: [0-9A-Fa-f]{8})+)")


def need_tools():
    if not (shutil.which("objcopy") and shutil.which("make") and os.path.exists(os.path.join(LLVM, "llvm-objdump"))):
        pytest.skip("binutils / ROCm LLVM tools not present")


def make_var(name):
    """A variable of the Makefile, as make expands it."""
    out = subprocess.check_output(["make", "-s", "-C", PKG, "--no-print-directory", "-pn", "build/flags.stamp"],
                                  text=True, stderr=subprocess.DEVNULL)
    m = re.search(rf"^{name} [:?]?= (.*)$", out, re.M)
    assert m, name
    return m.group(1).strip()


def disassemble(obj, tmp):
    """llvm-objdump of the gfx950 code object of `obj`: a host object with the bundle
    embedded, or a device-only object (then it is the code itself)."""
    tmp.mkdir(exist_ok=True)
    co = tmp / "k.co"
    fat = tmp / "fatbin.bin"
    subprocess.check_call(["objcopy", f"--dump-section=.hip_fatbin={fat}", obj, str(tmp / "copy.o")])
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={fat}",
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"])
    notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", str(co)], text=True)
    return subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", str(co)], text=True), notes


def hot_runs(dis, kernel):
    """The straight-line runs of >= 500 VALU instructions of a kernel, as test_codegen.py cuts
    them: lists of (address, size, mnemonic, operands)."""
    i = dis.index("<" + kernel)
    runs, cur = [], []
    for line in dis[i:dis.index("s_endpgm", i)].split("\n"):
        m = INSN.match(line)
        if not m:
            continue
        cur.append((int(m.group(3), 16), 4 * len(m.group(4).split()), m.group(1), m.group(2).strip()))
        if m.group(1).startswith(("s_cbranch", "s_branch")):
            runs.append(cur)
            cur = []
    runs.append(cur)
    return [r for r in runs if sum(op.startswith("v_") for _, _, op, _ in r) >= 500]


def counts(run):
    return (len(run), sum(op.startswith("v_") for _, _, op, _ in run), sum(op.startswith("s_") for _, _, op, _ in run))


def after_pin(run):
    """The instructions after the phase pin (`s_nop 0` at 0 mod 8 in the run's first tenth)."""
    for n, (addr, _, op, args) in enumerate(run[: max(len(run) // 10, 2)]):
        if op == "s_nop" and args == "0" and addr % 8 == 0:
            return run[n + 1:]
    raise AssertionError("no pin")


@pytest.fixture(scope="module")
def product(tmp_path_factory):
    need_tools()
    obj = os.path.join(PKG, "build", "kernels_plain.o")
    if not os.path.exists(obj):
        subprocess.check_call(["make", "-s", "-C", PKG, "build/kernels_plain.o"])
    return disassemble(obj, tmp_path_factory.mktemp("product"))


@pytest.fixture(scope="module")
def compiler(tmp_path_factory):
    """The same source with the same flags, straight from the compiler: no rewriter."""
    need_tools()
    tmp = tmp_path_factory.mktemp("compiler")
    obj = tmp / "kernels_plain.o"
    subprocess.check_call([make_var("HIPCC")] + make_var("HIPFLAGS").split() + make_var("PLAINFLAGS").split()
                          + ["-c", "csrc/kernels_plain.hip", "-o", str(obj)], cwd=PKG, stderr=subprocess.DEVNULL)
    return disassemble(str(obj), tmp / "d")


def kernel_name(J):
    return f"_ZN7gpuhash6k_scanILi{J}ELi0ELb0ELi0EE"


def shipped():
    js = [int(x) for x in make_var("UNIFORM_J").split()]
    assert js and 4 in js and set(js) <= set(range(14)), js   # config 2's kernel is among them
    return js


def test_every_valu_instruction_of_the_shipped_loops_is_8_bytes_at_4_mod_8(product):
    dis, _ = product
    for J in shipped():
        runs = hot_runs(dis, kernel_name(J))
        assert len(runs) == 1, (J, len(runs))
        body = after_pin(runs[0])
        valu = [(a, sz, op) for a, sz, op, _ in body if op.startswith("v_")]
        assert len(valu) >= 1000, (J, len(valu))          # the whole VALU body lies after the pin
        off = [(hex(a), sz, op) for a, sz, op in valu if sz != 8 or a % 8 != 4]
        assert not off, (J, len(off), off[:5])


def test_counts_opcodes_and_operands_are_the_compilers(product, compiler):
    """Nothing added, removed or reordered: per kernel the run's (instructions, VALU, SALU) is
    the compiler's, and instruction by instruction the opcode (up to the encoding suffix, and
    the right shift written as a bit-field extract) and the operands are too.  The kernels the
    Makefile does not list are the compiler's byte for byte."""
    dis, _ = product
    ref, _ = compiler
    js = shipped()
    for J in range(14):
        a, b = hot_runs(dis, kernel_name(J)), hot_runs(ref, kernel_name(J))
        assert len(a) == len(b) == 1, J
        a, b = a[0], b[0]
        assert counts(a) == counts(b), (J, counts(a), counts(b))
        if J not in js:
            assert [x[1:] for x in a] == [x[1:] for x in b], J
            continue
        changed = 0
        for (_, _, op, args), (_, _, rop, rargs) in zip(a, b):
            if (op, args) == (rop, rargs) or (op == rop and op.startswith(("s_cbranch", "s_branch"))):
                continue  # (a branch out of a longer body has another offset)
            changed += 1
            if rop == "s_lshr_b32":
                d, s, n = [t.strip() for t in rargs.split(",")]
                assert op == "s_bfe_u32" and args == f"{d}, {s}, {hex((32 - int(n)) << 16 | int(n))}", (J, op, args, rargs)
            else:
                assert rop.endswith("_e32") and op == rop[:-4] + "_e64" and args == rargs, (J, op, args, rop, rargs)
        assert changed >= 150, (J, changed)
    # the dump kernels (MODE 1) of the same unit are not touched
    dump = "_ZN7gpuhash6k_scanILi4ELi0ELb0ELi1EE"
    assert [[x[1:] for x in r] for r in hot_runs(dis, dump)] == [[x[1:] for x in r] for r in hot_runs(ref, dump)]


def test_config2_kernel_keeps_its_size_and_registers(product):
    dis, notes = product
    assert [counts(r) for r in hot_runs(dis, kernel_name(4))] == [(1271, 1196, 75)]
    meta = {}
    for block in notes.split("  - .")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        vg = re.search(r"\.vgpr_count:\s+(\d+)", block)
        sp = re.search(r"\.vgpr_spill_count:\s+(\d+)", block)
        if name and vg and sp:
            meta[name.group(1)] = (int(vg.group(1)), int(sp.group(1)))
    assert [v for n, v in meta.items() if "k_scanILi4ELi0ELb0ELi0E" in n] == [(64, 0)]


def test_tie_test_library_runs_the_same_rule(tmp_path):
    """libgpuhash_tietest.so's plain unit goes through the same steps, so the tie tests run the
    product's code path."""
    need_tools()
    obj = os.path.join(PKG, "build", "tie_kernels_plain.o")
    if not os.path.exists(obj):
        subprocess.check_call(["make", "-s", "-C", PKG, "build/tie_kernels_plain.o"])
    dis, _ = disassemble(obj, tmp_path / "tie")
    for J in shipped():
        (run,) = hot_runs(dis, kernel_name(J))
        assert all(sz == 8 and a % 8 == 4 for a, sz, op, _ in after_pin(run) if op.startswith("v_")), J


def test_collecting_kernel_held_against_config2_follows(tmp_path):
    """k_scan<4,0,false,3> of kernels_plain_collect.o (UNIFORM_J_COLLECT): a sparse collect is
    held to the cost of the search of the same range (test_gpu_collect_below.py), so its loop
    takes the same encoding; the unit's other kernels keep a 4-byte VALU encoding somewhere."""
    need_tools()
    js = [int(x) for x in make_var("UNIFORM_J_COLLECT").split()]
    assert 4 in js
    for stem in ("kernels_plain_collect", "tie_kernels_plain_collect"):
        obj = os.path.join(PKG, "build", stem + ".o")
        if not os.path.exists(obj):
            subprocess.check_call(["make", "-s", "-C", PKG, f"build/{stem}.o"])
        dis, _ = disassemble(obj, tmp_path / stem)
        for J in range(14):
            (run,) = hot_runs(dis, f"_ZN7gpuhash6k_scanILi{J}ELi0ELb0ELi3EE")
            uniform = all(sz == 8 and a % 8 == 4 for a, sz, op, _ in after_pin(run) if op.startswith("v_"))
            assert uniform == (J in js), (stem, J)
        if stem == "kernels_plain_collect":
            (run,) = hot_runs(dis, "_ZN7gpuhash6k_scanILi4ELi0ELb0ELi3EE")
            assert counts(run)[1] == 1196, counts(run)   # no more VALU than the search loop


def rewriter():
    if shutil.which("g++") is None or shutil.which("make") is None:
        pytest.skip("no host compiler")
    subprocess.check_call(["make", "-s", "-C", PKG, "build/phase_rewrite"])
    return os.path.join(PKG, "build", "phase_rewrite")


def test_fixture_rewrites_to_the_expected_text_and_assembles(tmp_path):
    """The hand-written snippet (a pinned block with plain, literal-carrying and SGPR-operand
    _e32 instructions, a compare writing vcc and a 4-byte scalar shift): the rewriter's output
    is the committed expected text, and it assembles for gfx950 with every VALU instruction of
    the selected kernel's loop at 4 mod 8 and the other kernel untouched."""
    out = tmp_path / "out.s"
    subprocess.check_call([rewriter(), "--min-valu", "8", "--kernel", "toy_loop", os.path.join(FIX, "fixture.s"), str(out)],
                          stdout=subprocess.DEVNULL)
    assert out.read_text() == open(os.path.join(FIX, "expected.s")).read()
    clang = os.path.join(LLVM, "clang")
    if not os.path.exists(clang):
        pytest.skip("ROCm LLVM tools not present")
    obj = tmp_path / "out.o"
    subprocess.check_call([clang, "-x", "assembler", "-target", "amdgcn-amd-amdhsa", "-mcpu=gfx950", "-c", str(out), "-o", str(obj)])
    dis = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", str(obj)], text=True)
    body = dis[dis.index("<toy_loop>"):dis.index("<toy_other>")]
    insns = [(int(m.group(3), 16), 4 * len(m.group(4).split()), m.group(1)) for m in map(INSN.match, body.split("\n")) if m]
    pin = next(n for n, (a, _, op) in enumerate(insns) if op == "s_nop" and a % 8 == 0)
    valu = [(a, sz, op) for a, sz, op in insns[pin + 1:] if op.startswith("v_")]
    assert len(valu) == 13 and all(sz == 8 and a % 8 == 4 for a, sz, _ in valu), valu
    assert "v_add_u32_e32 v3, 0x428a2f98, v1" in body and "s_bfe_u32 s9, s6, 0x1d0003" in body
    other = dis[dis.index("<toy_other>"):]
    assert "v_xor_b32_e32 v1, v1, v2" in other and "s_lshr_b32 s9, s6, 3" in other and "_e64" not in other


def test_rewriter_refuses_what_it_cannot_fix(tmp_path):
    """The build step exits non-zero and writes nothing: a kernel that is not there, and a loop
    whose odd 4-byte scalar instruction has no 8-byte form."""
    exe = rewriter()
    src = open(os.path.join(FIX, "fixture.s")).read()
    bad = tmp_path / "bad.s"
    bad.write_text(src.replace("s_lshr_b32 s9, s6, 3", "s_lshr_b32 s9, s6, s7"))
    for args, inp in [(["--kernel", "absent"], os.path.join(FIX, "fixture.s")), (["--kernel", "toy_loop"], str(bad))]:
        out = tmp_path / "o.s"
        r = subprocess.run([exe, "--min-valu", "8"] + args + [inp, str(out)], capture_output=True, text=True)
        assert r.returncode == 1 and "phase_rewrite:" in r.stderr and not out.exists(), (args, r.stderr)


def test_rewriter_stand_alone_under_asan_ubsan():
    """csrc/phase_rewrite_check_main.cpp: the parser and rewrite functions over the fixture and
    malformed inputs (truncated lines, a block with no pin, a literal-carrying _e32, bytes that
    are no assembly), in a program with its own main built with -fsanitize=address,undefined."""
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    subprocess.check_call(["make", "-s", "-C", PKG, "lib/phase_rewrite_asan"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(PKG, "lib", "phase_rewrite_asan"), os.path.join(FIX, "fixture.s"),
                        os.path.join(FIX, "expected.s")], env=env, capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and r.stdout.strip() == "ok", out[-4000:]
    assert "ERROR: AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
