// Host build of leg-kilo_amd/csrc/lk_relpose.h for tests/test_rpe_host.py - a program of its own:
//   g++ -O1 -g -ffp-contract=off -fsanitize=address,undefined -o relpose_host relpose_host.cc
//   relpose_host [file]      (without a file: standard input)
// A case is 48 numbers separated by white space, anything strtod reads (hexadecimal floats keep every bit): the estimate's pose i, its pose k, the
// ground truth's pose a, its pose b, each as nine row-major rotation entries and then three position coordinates.  Per case one line goes out:
// e_t, s, c of lk_relpose_eval as hexadecimal floats and e_r = atan2(s, c).  A trailing partial case is an error (exit status 2).
#include "../../leg-kilo_amd/csrc/lk_relpose.h"
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>

int main(int argc, char** argv) {
    FILE* f = argc > 1 ? fopen(argv[1], "r") : stdin;
    if (!f) {
        fprintf(stderr, "relpose_host: cannot open %s\n", argv[1]);
        return 2;
    }
    std::string text;
    char buf[4096];
    for (size_t n; (n = fread(buf, 1, sizeof(buf), f)) > 0;) text.append(buf, n);
    if (f != stdin) fclose(f);
    std::vector<double> v;
    const char* p = text.c_str();
    for (;;) {
        char* end = nullptr;
        const double x = strtod(p, &end);
        if (end == p) break;
        v.push_back(x);
        p = end;
    }
    while (*p == ' ' || *p == '\n' || *p == '\t' || *p == '\r') ++p;
    if (*p != '\0' || v.size() % 48 != 0) {
        fprintf(stderr, "relpose_host: %zu numbers read, a case is 48; unread text: '%.16s'\n", v.size(), p);
        return 2;
    }
    for (size_t k = 0; k < v.size(); k += 48) {
        const double* q = v.data() + k;
        double e_t, s, c;
        lk_relpose_eval(q, q + 9, q + 12, q + 21, q + 24, q + 33, q + 36, q + 45, &e_t, &s, &c);
        printf("%a %a %a %a\n", e_t, s, c, atan2(s, c));
    }
    return 0;
}
