// phase_rewrite_main.cpp -- build step between the device compile of a plain-kernel
// translation unit and its assembly (Makefile):
//   phase_rewrite [--min-valu N] --kernel PREFIX [--kernel PREFIX ...] in.s out.s
// rewrites the kernels whose names start with a PREFIX (phase_rewrite.h), verifies the result
// against the input, and writes it.  Any failure is a non-zero exit and no output file.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>

#include "phase_rewrite.h"

int main(int argc, char** argv) {
    phase_rewrite::Options opt;
    std::vector<std::string> files;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "--kernel") && i + 1 < argc) opt.prefixes.push_back(argv[++i]);
        else if (!strcmp(argv[i], "--min-valu") && i + 1 < argc) opt.min_valu = atoi(argv[++i]);
        else files.push_back(argv[i]);
    }
    if (files.size() != 2) {
        fprintf(stderr, "usage: phase_rewrite [--min-valu N] --kernel PREFIX ... in.s out.s\n");
        return 2;
    }
    std::ifstream f(files[0], std::ios::binary);
    if (!f) {
        fprintf(stderr, "phase_rewrite: cannot read %s\n", files[0].c_str());
        return 2;
    }
    std::stringstream ss;
    ss << f.rdbuf();
    const std::string in = ss.str();
    std::string out = in, err;
    std::vector<phase_rewrite::KernelReport> reports;
    if (!opt.prefixes.empty()) {  // no kernel selected: the compiler's text goes through as it is
        if (!phase_rewrite::rewrite(in, opt, out, reports, err) || !phase_rewrite::verify(in, out, opt, err)) {
            fprintf(stderr, "phase_rewrite: %s: %s\n", files[0].c_str(), err.c_str());
            return 1;
        }
    }
    for (const auto& k : reports)
        for (const auto& r : k.runs)
            printf("phase_rewrite: %.40s: run (%d, %d, %d) %s phase %d: %d VALU promoted, %d scalar widened\n",
                   k.name.c_str(), r.n, r.valu, r.salu, r.pinned ? "pinned" : "not pinned", r.phase, r.promoted,
                   r.widened);
    std::ofstream g(files[1], std::ios::binary);
    g << out;
    g.close();
    if (!g) {
        fprintf(stderr, "phase_rewrite: cannot write %s\n", files[1].c_str());
        return 2;
    }
    return 0;
}
