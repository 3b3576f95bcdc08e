// newton_check.cpp -- a stand-alone host check of the Newton rule (csrc/pu_newton.h).  Includes
// the header and nothing else of the library; tests/test_newton_reference.py records the script
// from tests/newton_reference.py, builds this program and runs it on the script.
//
// The script, all doubles as hex floats (or inf / -inf), one case after another:
//   case NAME T0 TOL MAX_ITER N      N evaluations follow
//   T LNL D1 D2                      the abscissa the rule must name, and what it is given there
//   end T LNL D1 D2 IT EVALS         the state the rule must end in
// Every abscissa and every end value must equal the recorded one bit for bit, and the rule must
// be done exactly when the record ends.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../phylo_utils_amd/csrc/pu_newton.h"

using namespace pu;

static int g_fail = 0;
static char g_case[128];
#define CHECK(cond, ...)                                    \
    do {                                                    \
        if (!(cond)) {                                      \
            ++g_fail;                                       \
            fprintf(stderr, "FAIL [%s] %s: ", g_case, #cond); \
            fprintf(stderr, __VA_ARGS__);                   \
            fprintf(stderr, "\n");                          \
        }                                                   \
    } while (0)

static bool same(double a, double b) {
    uint64_t x, y;
    memcpy(&x, &a, 8);
    memcpy(&y, &b, 8);
    return x == y;
}

// the next blank-separated word of the script as a double (strtod reads hex floats and inf)
static bool next_double(FILE *f, double *out) {
    char w[64], *end;
    if (fscanf(f, "%63s", w) != 1) return false;
    *out = strtod(w, &end);
    return end != w && *end == 0;
}

int main(int argc, char **argv) {
    if (argc != 2) return fprintf(stderr, "usage: newton_check SCRIPT\n"), 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return fprintf(stderr, "newton_check: cannot read %s\n", argv[1]), 2;
    int cases = 0, evals = 0;
    char word[16];
    while (fscanf(f, "%15s", word) == 1) {
        double t0, tol, r[4], e[4];
        int max_iter, n, it, ev;
        if (strcmp(word, "case") || fscanf(f, "%127s", g_case) != 1 || !next_double(f, &t0) ||
            !next_double(f, &tol) || fscanf(f, "%d %d", &max_iter, &n) != 2)
            return fprintf(stderr, "newton_check: malformed case header after %d cases\n", cases), 2;
        NewtonState s;
        double tn = newton_start(s, t0);
        for (int i = 0; i < n; ++i) {
            for (int k = 0; k < 4; ++k)
                if (!next_double(f, &r[k]))
                    return fprintf(stderr, "newton_check: [%s] malformed evaluation %d\n", g_case, i), 2;
            if (s.done) continue;  // reported once, below
            CHECK(same(tn, r[0]), "evaluation %d at %a, recorded %a", i, tn, r[0]);
            tn = newton_step(s, r[1], r[2], r[3], tol, max_iter);
            ++evals;
        }
        if (fscanf(f, "%15s", word) != 1 || strcmp(word, "end"))
            return fprintf(stderr, "newton_check: [%s] no end line\n", g_case), 2;
        for (int k = 0; k < 4; ++k)
            if (!next_double(f, &e[k]))
                return fprintf(stderr, "newton_check: [%s] malformed end line\n", g_case), 2;
        if (fscanf(f, "%d %d", &it, &ev) != 2)
            return fprintf(stderr, "newton_check: [%s] malformed end line\n", g_case), 2;
        CHECK(s.done && s.evals == n, "done = %d after %d of the %d recorded evaluations", s.done,
              s.evals, n);
        CHECK(same(s.tn, s.t), "tn = %a beside t = %a once done", s.tn, s.t);
        CHECK(same(s.t, e[0]) && same(s.lnl, e[1]) && same(s.d1, e[2]) && same(s.d2, e[3]),
              "end (%a, %a, %a, %a), recorded (%a, %a, %a, %a)", s.t, s.lnl, s.d1, s.d2, e[0], e[1],
              e[2], e[3]);
        CHECK(s.it == it && s.evals == ev, "it %d evals %d, recorded %d %d", s.it, s.evals, it, ev);
        ++cases;
    }
    fclose(f);
    printf("newton_check: %d cases, %d evaluations, %2d failures\n", cases, evals, g_fail);
    return g_fail ? 1 : 0;
}
