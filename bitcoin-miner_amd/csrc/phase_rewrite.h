// phase_rewrite.h -- puts every VALU instruction of a pinned per-nonce loop body at ONE code
// phase, by re-encoding alone.  Host-only; phase_rewrite_main.cpp is the build
// step, phase_rewrite_check_main.cpp the stand-alone sanitizer run of these functions.
//
// The loop bodies of the scan kernels mix 4-byte and 8-byte encodings, and every 4-byte
// instruction flips the phase (address mod 8) of everything after it, so the pin of
// scan_kernel.h (GPUHASH_LOOP_ALIGN) fixes the phase of the body's first instruction only.
// In the device assembly of a translation unit, for each selected kernel and each
// straight-line run of >= min_valu VALU instructions that opens with the pin, between the pin
// and the run's last VALU instruction:
//   * a 4-byte VALU encoding (`_e32` without a 32-bit literal) becomes its 8-byte VOP3 form
//     (`_e64`): same opcode, registers and operands.  An `_e32` that carries a literal is 8
//     bytes already, and gfx950's VOP3 takes no literal, so it stays.
//   * scalar instructions stay as they are where the 4-byte ones between two VALU
//     instructions come in pairs.  Where an odd one would flip the phase, one
//     `s_lshr_b32 D, S, n` of that group becomes `s_bfe_u32 D, S, (32-n) << 16 | n`: one
//     instruction for one, the same D, and the same SCC (both set it to D != 0).  A group
//     that holds no such shift cannot be fixed, and the rewrite of that kernel FAILS: nothing
//     is ever added, removed or reordered.
// Sizes come from mnemonics and operands alone (gfx9 encodings are 4 or 8 bytes), never from
// addresses.  verify() re-parses input and output and checks, independently of the rewrite's
// own bookkeeping, that the counts of every run are unchanged, that each instruction equals
// its original up to those two substitutions, and that every VALU instruction after a pin is
// 8 bytes at the pin's phase.
#pragma once
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

namespace phase_rewrite {

enum class LineKind { Blank, Comment, Directive, Label, Insn };

struct ParsedLine {
    LineKind kind = LineKind::Blank;
    std::string mnem;  // Insn: the mnemonic; Label: the name; Directive: the directive
    std::string ops;   // Insn, Directive: the operand text, comment and blanks stripped
};

inline bool starts_with(const std::string& s, const char* p) { return s.rfind(p, 0) == 0; }
inline bool ends_with(const std::string& s, const char* p) {
    const std::string q(p);
    return s.size() >= q.size() && s.compare(s.size() - q.size(), q.size(), q) == 0;
}

inline std::string trim(const std::string& s) {
    size_t b = 0, e = s.size();
    while (b < e && (s[b] == ' ' || s[b] == '\t' || s[b] == '\r')) b++;
    while (e > b && (s[e - 1] == ' ' || s[e - 1] == '\t' || s[e - 1] == '\r')) e--;
    return s.substr(b, e - b);
}

inline ParsedLine parse_line(const std::string& raw) {
    ParsedLine p;
    std::string s = raw;
    const size_t sc = s.find(';');  // a comment runs to the end of the line
    const bool had_comment = sc != std::string::npos;
    if (had_comment) s.erase(sc);
    s = trim(s);
    if (s.empty()) {
        p.kind = had_comment ? LineKind::Comment : LineKind::Blank;
        return p;
    }
    size_t e = 0;
    while (e < s.size() && s[e] != ' ' && s[e] != '\t') e++;
    const std::string head = s.substr(0, e);
    if (head.back() == ':') {
        p.kind = LineKind::Label;
        p.mnem = head.substr(0, head.size() - 1);
        return p;
    }
    p.kind = head[0] == '.' ? LineKind::Directive : LineKind::Insn;
    p.mnem = head;
    p.ops = trim(s.substr(e));
    return p;
}

// Operands at the top level of the text: commas inside [..] (register ranges, op_sel lists)
// and (..) do not split.
inline std::vector<std::string> split_operands(const std::string& ops) {
    std::vector<std::string> out;
    std::string cur;
    int depth = 0;
    for (char c : ops) {
        if (c == '[' || c == '(') depth++;
        if ((c == ']' || c == ')') && depth > 0) depth--;
        if (c == ',' && depth == 0) {
            out.push_back(trim(cur));
            cur.clear();
        } else {
            cur.push_back(c);
        }
    }
    if (!trim(cur).empty() || !out.empty()) out.push_back(trim(cur));
    return out;
}

// An integer operand, decimal or hex, with an optional sign.
inline bool parse_int(const std::string& t, long long& v) {
    if (t.empty()) return false;
    size_t i = (t[0] == '-' || t[0] == '+') ? 1 : 0;
    if (i >= t.size() || t[i] < '0' || t[i] > '9') return false;
    char* end = nullptr;
    errno = 0;
    const unsigned long long mag = std::strtoull(t.c_str() + i, &end, 0);
    if (!end || *end != '\0' || errno == ERANGE || mag > (1ull << 62)) return false;
    v = t[0] == '-' ? -(long long)mag : (long long)mag;
    return true;
}

// Does the operand take a 32-bit literal dword after the instruction?  Integers outside the
// inline range -16..64, floats other than the inline ones, and symbol expressions do.
inline bool is_literal_operand(const std::string& t) {
    long long v;
    if (parse_int(t, v)) return v < -16 || v > 64;
    if (t.empty()) return false;
    const size_t i = (t[0] == '-' || t[0] == '+') ? 1 : 0;
    if (i < t.size() && t[i] >= '0' && t[i] <= '9') {  // a float, or a number we cannot read
        static const char* const inl[] = {"0.5", "1.0", "2.0", "4.0", "0.15915494"};
        for (const char* f : inl)
            if (t.substr(i) == f) return t == "-0.15915494";
        return true;
    }
    return t[0] == '.' || t.find('@') != std::string::npos;  // .Lsym, sym@rel32@lo
}

inline bool has_literal(const std::string& ops) {
    for (const std::string& t : split_operands(ops))
        if (is_literal_operand(t)) return true;
    return false;
}

inline bool is_valu(const std::string& m) { return starts_with(m, "v_"); }
inline bool is_salu(const std::string& m) { return starts_with(m, "s_"); }
inline bool is_branch(const std::string& m) { return starts_with(m, "s_cbranch") || starts_with(m, "s_branch"); }

// Encoded size of a gfx9 instruction as the compiler prints it: 4 or 8 bytes.
inline int insn_bytes(const std::string& m, const std::string& ops) {
    if (is_valu(m)) {
        if (ends_with(m, "_e32")) return has_literal(ops) ? 8 : 4;
        if (ends_with(m, "_e64") || ends_with(m, "_dpp") || ends_with(m, "_sdwa")) return 8;
        // printed without a suffix: VOP1-only (4 bytes), the literal-carrying VOP2 forms, or
        // VOP3/VOP3P-only (8 bytes)
        static const char* const vop1_only[] = {"v_nop", "v_readfirstlane_b32", "v_clrexcp", "v_swap_b32"};
        for (const char* n : vop1_only)
            if (m == n) return 4;
        return 8;
    }
    if (is_salu(m)) {
        static const char* const smem[] = {"s_load_", "s_buffer_load_", "s_scratch_load_", "s_memtime",
                                           "s_memrealtime", "s_atc_probe", "s_setreg_imm32_b32"};
        for (const char* n : smem)
            if (starts_with(m, n)) return 8;
        // SOPP and SOPK: their immediate is in the instruction word
        static const char* const imm16[] = {"s_nop", "s_waitcnt", "s_branch", "s_cbranch", "s_endpgm", "s_barrier",
                                            "s_sleep", "s_sethalt", "s_setprio", "s_sendmsg", "s_trap",
                                            "s_icache_inv", "s_incperflevel", "s_decperflevel", "s_ttracedata",
                                            "s_setkill", "s_wakeup", "s_movk_i32", "s_cmovk_i32", "s_addk_i32",
                                            "s_mulk_i32", "s_cmpk_", "s_getreg_b32", "s_setreg_b32", "s_call_b64"};
        for (const char* n : imm16)
            if (starts_with(m, n)) return 4;
        return has_literal(ops) ? 8 : 4;  // SOP1, SOP2, SOPC
    }
    return 8;  // DS, FLAT/global/scratch, MUBUF
}

// The 8-byte VOP3 form of a 4-byte `_e32` VALU instruction: the same text with `_e64`.
inline bool promote_valu(const std::string& m, const std::string& ops, std::string& out) {
    if (!is_valu(m) || !ends_with(m, "_e32") || has_literal(ops)) return false;
    out = m.substr(0, m.size() - 4) + "_e64";
    return true;
}

// The 8-byte form of a 4-byte scalar right shift by an immediate: a bit-field extract of
// the 32 - n bits from bit n.  D and SCC (D != 0) come out the same.
inline bool widen_scalar(const std::string& m, const std::string& ops, std::string& om, std::string& oo) {
    if (m != "s_lshr_b32") return false;
    const std::vector<std::string> t = split_operands(ops);
    long long n;
    if (t.size() != 3 || !parse_int(t[2], n) || n < 1 || n > 31) return false;
    if (is_literal_operand(t[1]) || t[0].empty() || t[1].empty()) return false;
    char lit[16];
    snprintf(lit, sizeof lit, "0x%x", (unsigned)(((32 - n) << 16) | n));
    om = "s_bfe_u32";
    oo = t[0] + ", " + t[1] + ", " + lit;
    return true;
}

struct RunReport {
    int n = 0, valu = 0, salu = 0;
    bool pinned = false;
    int phase = -1;                   // of the instruction after the pin: 0 or 4
    int promoted = 0, widened = 0;    // VALU `_e32` -> `_e64`; scalar shifts -> bit-field extracts
};
struct KernelReport {
    std::string name;
    std::vector<RunReport> runs;      // the runs of >= min_valu VALU instructions
};
struct Options {
    std::vector<std::string> prefixes;  // kernels whose name starts with one of these
    int min_valu = 500;
};

namespace detail {

struct Insn {
    size_t line;
    std::string mnem, ops;
};
struct Run {
    std::vector<Insn> insns;
    long pin = -1;   // index of the first instruction after the pin, -1: none
    int phase = -1;
};
struct Kernel {
    std::string name;
    std::vector<Run> runs;
};

inline bool selected(const std::string& name, const Options& o) {
    for (const std::string& p : o.prefixes)
        if (starts_with(name, p.c_str())) return true;
    return false;
}

inline std::vector<std::string> split_lines(const std::string& text) {
    std::vector<std::string> lines;
    size_t b = 0;
    while (b <= text.size()) {
        size_t e = text.find('\n', b);
        if (e == std::string::npos) {
            if (b < text.size()) lines.push_back(text.substr(b));
            break;
        }
        lines.push_back(text.substr(b, e - b));
        b = e + 1;
    }
    return lines;
}

// The selected kernels of a translation unit, cut into runs at the branches.  A pin is a
// `.p2align 3` directive, with the `s_nop 0` after it if there is one (phase 4; without, 0);
// it counts for a run if it lies in the run's first tenth.
inline bool scan(const std::vector<std::string>& lines, const Options& o, std::vector<Kernel>& ks,
                 std::string& err) {
    size_t i = 0;
    while (i < lines.size()) {
        const ParsedLine h = parse_line(lines[i]);
        const bool top = !lines[i].empty() && lines[i][0] != ' ' && lines[i][0] != '\t';
        if (!(top && h.kind == LineKind::Label && selected(h.mnem, o))) {
            i++;
            continue;
        }
        Kernel k;
        k.name = h.mnem;
        Run cur;
        std::vector<size_t> pins;  // instruction index (within cur) a pin directive precedes
        bool ended = false;
        auto close = [&]() {
            const size_t head = cur.insns.size() / 10 > 2 ? cur.insns.size() / 10 : 2;
            for (size_t p : pins) {
                if (p >= head || p >= cur.insns.size()) continue;
                const Insn& a = cur.insns[p];
                if (a.mnem == "s_nop" && a.ops == "0") {
                    cur.pin = (long)p + 1;
                    cur.phase = 4;
                } else {
                    cur.pin = (long)p;
                    cur.phase = 0;
                }
                break;
            }
            k.runs.push_back(cur);
            cur = Run{};
            pins.clear();
        };
        for (i++; i < lines.size(); i++) {
            const ParsedLine p = parse_line(lines[i]);
            if (p.kind == LineKind::Directive && p.mnem == ".p2align" && p.ops == "3") pins.push_back(cur.insns.size());
            if (p.kind != LineKind::Insn) continue;
            if (p.mnem == "s_endpgm") {
                ended = true;
                break;
            }
            cur.insns.push_back(Insn{i, p.mnem, p.ops});
            if (is_branch(p.mnem)) close();
        }
        if (!ended) {
            err = "kernel " + k.name + ": no s_endpgm before the end of the input";
            return false;
        }
        close();
        ks.push_back(k);
    }
    return true;
}

inline void count(const Run& r, RunReport& rep) {
    rep.n = (int)r.insns.size();
    rep.valu = rep.salu = 0;
    for (const Insn& x : r.insns) {
        rep.valu += is_valu(x.mnem);
        rep.salu += is_salu(x.mnem);
    }
}

}  // namespace detail

// Rewrites the selected kernels of `in` into `out`.  False with `err` set if a selected kernel
// is missing, has no pinned run, or has a run that cannot be brought to one phase.
inline bool rewrite(const std::string& in, const Options& o, std::string& out,
                    std::vector<KernelReport>& reports, std::string& err) {
    using namespace detail;
    std::vector<std::string> lines = split_lines(in);
    std::vector<Kernel> ks;
    if (!scan(lines, o, ks, err)) return false;
    for (const std::string& p : o.prefixes) {
        int hits = 0;
        for (const Kernel& k : ks) hits += starts_with(k.name, p.c_str());
        if (hits != 1) {
            err = "kernel prefix " + p + ": " + std::to_string(hits) + " kernels match";
            return false;
        }
    }
    for (const Kernel& k : ks) {
        KernelReport kr;
        kr.name = k.name;
        int pinned = 0;
        for (const Run& r : k.runs) {
            RunReport rep;
            count(r, rep);
            if (rep.valu < o.min_valu) continue;
            rep.pinned = r.pin >= 0;
            rep.phase = r.phase;
            if (rep.pinned) {
                pinned++;
                long last = -1;
                for (long j = (long)r.insns.size() - 1; j >= r.pin; j--)
                    if (is_valu(r.insns[j].mnem)) { last = j; break; }
                int phase = r.phase;
                long group = r.pin;  // first instruction after the previous VALU one
                std::vector<bool> wide(r.insns.size(), false);
                for (long j = r.pin; j <= last; j++) {
                    const Insn& x = r.insns[j];
                    if (!is_valu(x.mnem)) {
                        phase = (phase + insn_bytes(x.mnem, x.ops)) & 7;
                        continue;
                    }
                    if (insn_bytes(x.mnem, x.ops) == 4) {
                        std::string m;
                        if (!promote_valu(x.mnem, x.ops, m)) {
                            err = "kernel " + k.name + ": no 8-byte form of `" + x.mnem + " " + x.ops + "`";
                            return false;
                        }
                        lines[x.line] = "\t" + m + " " + x.ops;
                        rep.promoted++;
                    }
                    if (phase != r.phase) {  // an odd 4-byte scalar since the last VALU instruction
                        bool done = false;
                        for (long g = group; g < j && !done; g++) {
                            const Insn& y = r.insns[g];
                            std::string m, ops;
                            if (wide[g] || insn_bytes(y.mnem, y.ops) != 4 || !widen_scalar(y.mnem, y.ops, m, ops)) continue;
                            lines[y.line] = "\t" + m + " " + ops;
                            wide[g] = true;
                            rep.widened++;
                            phase = (phase + 4) & 7;
                            done = true;
                        }
                        if (!done) {
                            err = "kernel " + k.name + ": `" + x.mnem + " " + x.ops + "` (instruction " +
                                  std::to_string(j) + " of its run) is off phase and no scalar instruction before it can be widened";
                            return false;
                        }
                    }
                    group = j + 1;
                }
            }
            kr.runs.push_back(rep);
        }
        if (!pinned) {
            err = "kernel " + k.name + ": no pinned run of >= " + std::to_string(o.min_valu) + " VALU instructions";
            return false;
        }
        reports.push_back(kr);
    }
    out.clear();
    for (const std::string& l : lines) {
        out += l;
        out += '\n';
    }
    return true;
}

// Checks `out` against `in` from the texts alone (see the head of this file).
inline bool verify(const std::string& in, const std::string& out, const Options& o, std::string& err) {
    using namespace detail;
    const std::vector<std::string> li = split_lines(in), lo = split_lines(out);
    std::vector<Kernel> ki, ko;
    if (!scan(li, o, ki, err) || !scan(lo, o, ko, err)) return false;
    if (ki.size() != ko.size() || ki.size() != o.prefixes.size()) {
        err = "verify: " + std::to_string(ki.size()) + " kernels in, " + std::to_string(ko.size()) + " out, " +
              std::to_string(o.prefixes.size()) + " asked for";
        return false;
    }
    for (size_t k = 0; k < ki.size(); k++) {
        const Kernel &a = ki[k], &b = ko[k];
        const std::string where = "verify: kernel " + a.name + ": ";
        if (a.name != b.name || a.runs.size() != b.runs.size()) {
            err = where + "kernels or their runs differ";
            return false;
        }
        int pinned = 0;
        for (size_t r = 0; r < a.runs.size(); r++) {
            const Run &x = a.runs[r], &y = b.runs[r];
            RunReport cx, cy;
            count(x, cx);
            count(y, cy);
            if (cx.n != cy.n || cx.valu != cy.valu || cx.salu != cy.salu || x.pin != y.pin || x.phase != y.phase) {
                err = where + "run " + std::to_string(r) + " changed its instruction counts or its pin";
                return false;
            }
            for (size_t j = 0; j < x.insns.size(); j++) {
                const Insn &p = x.insns[j], &q = y.insns[j];
                if (p.mnem == q.mnem && p.ops == q.ops) continue;
                std::string m, ops;
                const bool inside = x.pin >= 0 && (long)j >= x.pin && cx.valu >= o.min_valu;
                if (inside && promote_valu(p.mnem, p.ops, m) && m == q.mnem && p.ops == q.ops) continue;
                if (inside && widen_scalar(p.mnem, p.ops, m, ops) && m == q.mnem && ops == q.ops) continue;
                err = where + "`" + p.mnem + " " + p.ops + "` became `" + q.mnem + " " + q.ops + "`";
                return false;
            }
            if (cy.valu < o.min_valu || y.pin < 0) continue;
            pinned++;
            int phase = y.phase;
            long last = -1;
            for (long j = (long)y.insns.size() - 1; j >= y.pin; j--)
                if (is_valu(y.insns[j].mnem)) { last = j; break; }
            for (long j = y.pin; j <= last; j++) {
                const Insn& q = y.insns[j];
                const int bytes = insn_bytes(q.mnem, q.ops);
                if (is_valu(q.mnem) && (bytes != 8 || phase != y.phase)) {
                    err = where + "`" + q.mnem + " " + q.ops + "` is " + std::to_string(bytes) + " bytes at phase " +
                          std::to_string(phase) + ", the pin's is " + std::to_string(y.phase);
                    return false;
                }
                phase = (phase + bytes) & 7;
            }
        }
        if (!pinned) {
            err = where + "no pinned run";
            return false;
        }
    }
    return true;
}

}  // namespace phase_rewrite
