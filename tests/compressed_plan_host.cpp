// Host program of tests/test_compressed_plan.py: slmsuite_amd/csrc/compressed_plan.hpp without a GPU.
//   cases  one case per line of stdin -> one JSON object per line (numbers may be hexadecimal floats):
//            terms  <sep_maxdeg> px py px py ...                     classification of a term list
//            slots  <M> <px py> x M  <coefficients> x M              canonical coefficients of one spot
//            grid   f32|f64 <axis> <H> <W> <values> x H*W            product-grid test and the axis taken
//            axis   <W> <values> x W                                 regular-grid test
//            chunks <N> <n_cu> <run_blocks>                          spot chunks of the run kernels
//            form   elem sep_valid run_valid opt_separable opt_sep_min opt_run n_spots n_monomials degree mono_tab c_mtab
//   sweep  the form choice over the whole product of its facts, the invariants checked on every point
//          -> "violation ..." lines, then "checked N violations K"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include "compressed_plan.hpp"

using namespace hgs;

static const char* form_name(CForm f) { return f == CForm::sep_gemm ? "sep_gemm" : f == CForm::run ? "run" : "pixel"; }

template <typename T> static void grid_case(std::istringstream& in) {
    int axis = 0, H = 0, W = 0;
    in >> axis >> H >> W;
    std::vector<T> h((size_t)H * W);
    std::string tok;
    for (T& v : h) { in >> tok; v = (T)strtod(tok.c_str(), nullptr); }
    std::vector<double> out;
    const bool sep = product_grid_axis(h.data(), H, W, axis, out);
    printf("{\"sep\": %d, \"axis\": [", sep);
    for (size_t i = 0; i < out.size(); ++i) printf("%s%.17g", i ? ", " : "", out[i]);
    printf("]}\n");
}

static int cases() {
    char buf[1 << 16];
    while (fgets(buf, sizeof buf, stdin)) {
        std::istringstream in(buf);
        std::string what, tok;
        if (!(in >> what)) continue;
        if (what == "terms") {
            int maxdeg = 0, v = 0;
            in >> maxdeg;
            std::vector<int32_t> mono;
            while (in >> v) mono.push_back(v);
            const TermClass t = classify_terms(mono.data(), (int)mono.size() / 2, maxdeg);
            printf("{\"degree\": %d, \"bad\": %d, \"separable\": %d, \"dx\": %d, \"dy\": %d}\n", t.degree, t.bad, t.separable, t.dx, t.dy);
        } else if (what == "slots") {
            int M = 0;
            in >> M;
            std::vector<int32_t> mono((size_t)2 * M);
            std::vector<float> coeff((size_t)M);
            for (int32_t& v : mono) in >> v;
            for (float& v : coeff) { in >> tok; v = (float)strtod(tok.c_str(), nullptr); }
            double c[6] = {0, 0, 0, 0, 0, 0};
            canonical_coeffs(mono.data(), M, coeff.data(), 1, 0, c);
            printf("{\"c\": [%.17g, %.17g, %.17g, %.17g, %.17g, %.17g]}\n", c[0], c[1], c[2], c[3], c[4], c[5]);
        } else if (what == "grid") {
            in >> tok;
            if (tok == "f32") grid_case<float>(in); else grid_case<double>(in);
        } else if (what == "axis") {
            int W = 0;
            in >> W;
            std::vector<double> xs((size_t)W);
            for (double& v : xs) { in >> tok; v = strtod(tok.c_str(), nullptr); }
            const RegularAxis r = regular_axis(xs.data(), W);
            printf("{\"ok\": %d, \"x0\": %.17g, \"hx\": %.17g}\n", r.ok, r.x0, r.hx);
        } else if (what == "chunks") {
            int N = 0, n_cu = 0, run_blocks = 0;
            in >> N >> n_cu >> run_blocks;
            const RunChunks c = run_chunking(N, n_cu, run_blocks);
            printf("{\"nper\": %d, \"chunks\": %d}\n", c.nper, c.chunks);
        } else if (what == "form") {
            CFormFacts f;
            int sep_valid = 0, run_valid = 0;
            in >> f.elem >> sep_valid >> run_valid >> f.opt_separable >> f.opt_sep_min >> f.opt_run >> f.n_spots >> f.n_monomials >>
                f.degree >> f.mono_tab >> f.c_mtab;
            f.sep_valid = sep_valid != 0;
            f.run_valid = run_valid != 0;
            const CFormChoice c = choose_form(f);
            printf("{\"form\": \"%s\", \"deg\": %d}\n", form_name(c.form), c.deg);
        } else {
            fprintf(stderr, "unknown case %s\n", what.c_str());
            return 2;
        }
    }
    return 0;
}

static long n_checked = 0, n_bad = 0;
static void violation(const char* what, const CFormFacts& f, const CFormChoice& c) {
    if (++n_bad > 40) return;
    printf("violation: %s | elem=%d sep_valid=%d run_valid=%d opt_separable=%d opt_sep_min=%d opt_run=%d n_spots=%d n_monomials=%d degree=%d "
           "mono_tab=%d c_mtab=%d -> %s deg %d\n", what, f.elem, f.sep_valid, f.run_valid, f.opt_separable, f.opt_sep_min, f.opt_run, f.n_spots,
           f.n_monomials, f.degree, f.mono_tab, f.c_mtab, form_name(c.form), c.deg);
}

// each invariant is a guard of the engine before the plan existed (use_sep, use_run, the four-way chain by degree)
static int sweep() {
    for (int elem : {4, 8})
    for (int sep_valid : {0, 1})
    for (int run_valid : {0, 1})
    for (int opt_separable : {0, 1})
    for (int opt_sep_min : {1, 96, 200})
    for (int opt_run : {0, 1})
    for (int n_spots : {1, 40, 95, 96, 120, 199, 200, 10000})
    for (int n_monomials : {1, 2, 3, 6, 15, 16, 17, 40})
    for (int degree : {0, 1, 2, 3, 4, 8})
    for (int mono_tab : {0, 1}) {
        CFormFacts f;
        f.elem = elem; f.sep_valid = sep_valid != 0; f.run_valid = run_valid != 0; f.opt_separable = opt_separable;
        f.opt_sep_min = opt_sep_min; f.opt_run = opt_run; f.n_spots = n_spots; f.n_monomials = n_monomials; f.degree = degree;
        f.mono_tab = mono_tab; f.c_mtab = 16;
        const CFormChoice c = choose_form(f), inverse = choose_form(f);      // n2f and f2n: the same call
        ++n_checked;
        if (!(c == inverse)) violation("the two directions disagree", f, c);
        if (elem != 4 && c.form != CForm::pixel) violation("fp64 outside the per-pixel kernels", f, c);
        const bool sep_may = elem == 4 && sep_valid && opt_separable && n_spots >= opt_sep_min;
        const bool run_may = elem == 4 && run_valid && opt_run && degree <= 2;
        if ((c.form == CForm::sep_gemm) != sep_may) violation("separable form and its preconditions disagree", f, c);
        if ((c.form == CForm::run) != (!sep_may && run_may)) violation("run form and its preconditions disagree", f, c);
        if ((c.form == CForm::pixel) != (!sep_may && !run_may)) violation("per-pixel form although another applies (or the reverse)", f, c);
        if (c.form == CForm::run && c.deg != (degree <= 1 ? 1 : 2)) violation("run instance", f, c);
        if (c.form == CForm::pixel) {
            const int want = degree <= 1 ? 1 : degree == 2 ? 2 : (n_monomials <= f.c_mtab && mono_tab) ? 3 : 0;
            if (c.deg != want) violation("per-pixel instance", f, c);
            if (c.deg == 3 && !(n_monomials <= f.c_mtab && mono_tab)) violation("monomial table beyond its size or switched off", f, c);
        }
    }
    printf("checked %ld violations %ld\n", n_checked, n_bad);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "cases")) return cases();
    if (argc == 2 && !strcmp(argv[1], "sweep")) return sweep();
    fprintf(stderr, "usage: %s cases|sweep\n", argv[0]);
    return 2;
}
