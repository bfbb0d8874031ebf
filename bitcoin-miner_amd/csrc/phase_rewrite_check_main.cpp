// phase_rewrite_check_main.cpp -- test-only: the parser and rewrite functions of
// phase_rewrite.h in a stand-alone program, built with -fsanitize=address,undefined
// (lib/phase_rewrite_asan; tests/test_codegen_uniform_phase.py runs it):
//   phase_rewrite_asan fixture.s expected.s
// rewrites the hand-written fixture and compares it with the expected text, then feeds the
// functions malformed inputs, each of which must be refused with a message and nothing else.
// Prints "ok" and exits 0 if everything held.
#include <cstdio>
#include <fstream>
#include <sstream>

#include "phase_rewrite.h"

using namespace phase_rewrite;

static int failures = 0;
#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            fprintf(stderr, "line %d: failed: %s\n", __LINE__, #c);   \
            failures++;                                              \
        }                                                            \
    } while (0)

static std::string slurp(const char* path) {
    std::ifstream f(path, std::ios::binary);
    std::stringstream ss;
    ss << f.rdbuf();
    return ss.str();
}

static std::string replaced(std::string s, const std::string& a, const std::string& b) {
    const size_t p = s.find(a);
    if (p == std::string::npos) {
        fprintf(stderr, "the fixture lost `%s`\n", a.c_str());
        failures++;
        return s;
    }
    return s.replace(p, a.size(), b);
}

// rewrite + verify as the build step runs them
static bool run(const std::string& in, const Options& o, std::string& out, std::string& err) {
    std::vector<KernelReport> rep;
    out.clear();
    err.clear();
    return rewrite(in, o, out, rep, err) && verify(in, out, o, err);
}

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: phase_rewrite_asan fixture.s expected.s\n");
        return 2;
    }
    const std::string fix = slurp(argv[1]), want = slurp(argv[2]);
    CHECK(!fix.empty() && !want.empty());
    Options o;
    o.prefixes = {"toy_loop"};
    o.min_valu = 8;
    std::string out, err;

    // ---- line level ----
    CHECK(parse_line("").kind == LineKind::Blank);
    CHECK(parse_line("\t; only a comment").kind == LineKind::Comment);
    CHECK(parse_line(".LBB0_1:   ; x").kind == LineKind::Label && parse_line(".LBB0_1:").mnem == ".LBB0_1");
    CHECK(parse_line("\t.p2align 3").kind == LineKind::Directive && parse_line("\t.p2align 3").ops == "3");
    CHECK(parse_line("\tv_add_u32_e32 v1, v2, v3 ; c").ops == "v1, v2, v3");
    CHECK(parse_line("\tv_add_u32_e32").kind == LineKind::Insn && parse_line("\tv_add_u32_e32").ops.empty());
    CHECK(parse_line("v").mnem == "v" && parse_line(":").kind == LineKind::Label);
    CHECK(split_operands("").empty() && split_operands("v1,").size() == 2 && split_operands(",").size() == 2);
    CHECK(split_operands("v[1:2], s[0:1], 0x10").size() == 3);
    CHECK(split_operands("v1, v2 op_sel:[0,1]").size() == 2 && split_operands("]]],[[").size() == 2);
    CHECK(!is_literal_operand("64") && is_literal_operand("65") && !is_literal_operand("-16") && is_literal_operand("-17"));
    CHECK(is_literal_operand("0x30303030") && !is_literal_operand("0x10") && !is_literal_operand("1.0") &&
          is_literal_operand("3.0") && is_literal_operand("0x") && is_literal_operand("99999999999999999999999"));
    CHECK(!is_literal_operand("v1") && !is_literal_operand("vcc") && !is_literal_operand("") && !is_literal_operand("-") &&
          is_literal_operand(".Lsym") && is_literal_operand("sym@rel32@lo+4"));
    CHECK(insn_bytes("v_add_u32_e32", "v1, v2, v3") == 4 && insn_bytes("v_add_u32_e32", "v1, 0x428a2f98, v3") == 8);
    CHECK(insn_bytes("v_alignbit_b32", "v1, v2, v3, 7") == 8 && insn_bytes("v_readfirstlane_b32", "s1, v1") == 4);
    CHECK(insn_bytes("s_lshr_b32", "s1, s0, 3") == 4 && insn_bytes("s_mov_b32", "s0, 0x240ca1cc") == 8);
    CHECK(insn_bytes("s_load_dword", "s11, s[70:71], 0x10") == 8 && insn_bytes("s_waitcnt", "lgkmcnt(0)") == 4);
    CHECK(insn_bytes("s_movk_i32", "s0, 0x1000") == 4 && insn_bytes("global_load_dword", "v1, v[2:3], off") == 8);
    std::string m, ops;
    CHECK(promote_valu("v_xor_b32_e32", "v1, s9, v1", m) && m == "v_xor_b32_e64");
    CHECK(!promote_valu("v_add_u32_e32", "v3, 0x428a2f98, v1", m));  // literal-carrying _e32
    CHECK(!promote_valu("v_alignbit_b32", "v1, v2, v3, 7", m) && !promote_valu("_e32", "", m) && !promote_valu("", "", m));
    CHECK(widen_scalar("s_lshr_b32", "s1, s0, 3", m, ops) && m == "s_bfe_u32" && ops == "s1, s0, 0x1d0003");
    CHECK(widen_scalar("s_lshr_b32", "s1, s0, 31", m, ops) && ops == "s1, s0, 0x1001f");
    CHECK(!widen_scalar("s_lshr_b32", "s1, s0, s2", m, ops) && !widen_scalar("s_lshr_b32", "s1, s0, 32", m, ops) &&
          !widen_scalar("s_lshr_b32", "s1, s0", m, ops) && !widen_scalar("s_lshr_b32", "", m, ops) &&
          !widen_scalar("s_lshr_b32", "s1, 0x12345, 3", m, ops) && !widen_scalar("s_lshl_b32", "s1, s0, 3", m, ops));

    // ---- the fixture ----
    CHECK(run(fix, o, out, err));
    CHECK(out == want);
    if (out != want) fprintf(stderr, "rewritten fixture:\n%s\nerror: %s\n", out.c_str(), err.c_str());
    {   // the kernel that was not selected is unchanged, and a rewritten text is a fixed point
        const size_t a = fix.find("toy_other:"), b = out.find("toy_other:");
        CHECK(a != std::string::npos && b != std::string::npos && fix.substr(a) == out.substr(b));
        std::string again;
        CHECK(run(out, o, again, err) && again == out);
    }
    {   // the phase-0 control: the pin without its s_nop
        std::string out0;
        CHECK(run(replaced(fix, "\t.p2align 3\n\ts_nop 0\n", "\t.p2align 3\n"), o, out0, err));
        CHECK(out0.find("v_xor_b32_e64 v1, s9, v1") != std::string::npos && out0.find("s_bfe_u32") != std::string::npos);
    }

    // ---- malformed inputs: refused, with a message ----
    CHECK(!run("", o, out, err) && !err.empty());
    CHECK(!run("toy_loop:\n\tv_add_u32_e32 v1, v2", o, out, err) && !err.empty());  // truncated: no s_endpgm
    CHECK(!run(fix.substr(0, fix.find("s_cbranch_scc0")), o, out, err) && err.find("s_endpgm") != std::string::npos);
    CHECK(!run(fix.substr(0, fix.find("v_cmp_le_u32_e32") + 9), o, out, err) && !err.empty());  // cut inside a line
    CHECK(!run(replaced(fix, "\t.p2align 3\n\ts_nop 0\n", ""), o, out, err) &&  // a block with no pin
          err.find("no pinned run") != std::string::npos);
    // the odd scalar cannot be widened: a shift by a register, and a shift whose source is a literal
    CHECK(!run(replaced(fix, "s_lshr_b32 s9, s6, 3", "s_lshr_b32 s9, s6, s7"), o, out, err) &&
          err.find("off phase") != std::string::npos);
    // ... a literal-carrying shift is 8 bytes: then the PAIR after it is what keeps the phase
    CHECK(run(replaced(fix, "s_lshr_b32 s9, s6, 3", "s_lshr_b32 s9, 0x12345, 3"), o, out, err));
    // a VALU instruction with no 8-byte form
    CHECK(!run(replaced(fix, "v_mov_b32_e32 v8, s12", "v_readfirstlane_b32 s12, v8"), o, out, err) &&
          err.find("no 8-byte form") != std::string::npos);
    // a literal-carrying _e32 stays, whatever surrounds it
    CHECK(run(replaced(fix, "v_add_u32_e32 v4, v3, v0", "v_add_u32_e32 v4, 0x12345678, v0"), o, out, err) &&
          out.find("v_add_u32_e32 v4, 0x12345678, v0") != std::string::npos);
    {   // kernel selection: none, two of one prefix, a missing one
        Options p = o;
        p.prefixes = {"toy_"};
        CHECK(!run(fix, p, out, err) && err.find("2 kernels match") != std::string::npos);
        p.prefixes = {"toy_loop", "absent"};
        CHECK(!run(fix, p, out, err) && err.find("0 kernels match") != std::string::npos);
        p.prefixes = {"toy_loop"};
        p.min_valu = 500;  // the run is too short to count
        CHECK(!run(fix, p, out, err) && err.find("no pinned run") != std::string::npos);
    }
    // verify() on its own refuses an output that lost, gained or changed an instruction
    CHECK(!verify(fix, replaced(want, "\tv_mov_b32_e64 v8, s12\n", ""), o, err));
    CHECK(!verify(fix, replaced(want, "\tv_mov_b32_e64 v8, s12\n", "\tv_mov_b32_e64 v8, s12\n\ts_nop 0\n\ts_nop 0\n"), o, err));
    CHECK(!verify(fix, replaced(want, "v_mov_b32_e64 v8, s12", "v_mov_b32_e64 v8, s11"), o, err));
    CHECK(!verify(fix, replaced(want, "s_bfe_u32 s9, s6, 0x1d0003", "s_bfe_u32 s9, s6, 0x1c0003"), o, err));
    CHECK(!verify(fix, fix, o, err) && err.find("4 bytes") != std::string::npos);  // not rewritten at all
    CHECK(verify(fix, want, o, err));
    // bytes that are no assembly at all
    CHECK(!run(std::string("toy_loop:\n\0\xff\xfe\n\t\t\t,,,[[[\n", 24), o, out, err));

    if (failures) return 1;
    puts("ok");
    return 0;
}
