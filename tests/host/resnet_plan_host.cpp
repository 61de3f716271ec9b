// resnet_plan_host.cpp -- the verifier's launch planner (salve_amd/csrc/resnet_plan.h), compiled for the HOST from the very header
// resnet.hip includes, as a stand-alone program: tests/test_resnet_plan_host.py builds it with g++ (-O2, and -O1 -g
// -fsanitize=address,undefined -fno-sanitize-recover=all), runs it as a child process and pins what it prints.
//
//   resnet_plan_host IN
// IN:  int32 programs; per program: int32 n_ops, int32 ktab_entries, int32 n_flags, int32 n_queries, n_ops x salve_resnet_op_t,
//      ktab_entries x int32, n_flags x int32 flags, n_queries x {int32 flags, int32 op, int32 batch}.
// OUT (text): per program p and flags f one line   "P p F f: first+count:token ..."   -- the steps in order -- or
//      "P p F f: REFUSED message"; per query one line   "Q p f op batch: 0|1"   -- conv_runs_wide of the step that starts at that op
//      (-1 if none does or it is no CONV step).
// The ops and the k table live in heap blocks of exactly their size: a planner that looks past either end ends the program.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../salve_amd/csrc/resnet_plan.h"

static const char* g_message = "";
bool salve_fail(const char* msg) {
    g_message = msg;
    return false;
}

using namespace salve_plan;

static std::string token(const Step& st) {
    static const char* const chain[] = {"x128", "x256", "c128_128", "c128_256", "c256_256", "x256_split", "c128_256_split", "c256_256_split", "x128_w16", "c128_128_w16"};
    static const char* const block[] = {"block", "block_proj", "block_next"};
    std::string t;
    switch (st.kind) {
    case STEM_POOL: t = "stem"; break;
    case BOTTLENECK: t = block[st.form]; break;
    case EXPAND_CHAIN: t = chain[st.form]; break;
    case CONV: t = st.form == WIDE_OFF ? "conv" : (st.form == WIDE_8PHASE ? (st.wide_auto ? "conv8_auto" : "conv8") : "wide" + std::to_string(st.form)); break;
    case MAXPOOL: t = "maxpool"; break;
    case AVGPOOL_FC: t = "fc"; break;
    }
    if (st.kind == EXPAND_CHAIN && st.chained != (st.count == 2)) t += "!chained";
    if (st.y_even) t += "_even";
    return std::to_string(st.first) + "+" + std::to_string(st.count) + ":" + t;
}

static bool read_all(FILE* f, void* dst, size_t n) { return n == 0 || fread(dst, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s IN\n", argv[0]);
        return 2;
    }
    FILE* in = fopen(argv[1], "rb");
    if (!in) {
        fprintf(stderr, "cannot open %s\n", argv[1]);
        return 2;
    }
    int32_t programs = 0;
    if (!read_all(in, &programs, 4) || programs < 0) return 2;
    for (int32_t p = 0; p < programs; p++) {
        int32_t head[4];
        if (!read_all(in, head, sizeof head) || head[0] < 0 || head[1] < 0 || head[2] < 0 || head[3] < 0) return 2;
        std::vector<salve_resnet_op_t> ops((size_t)head[0]);
        std::vector<int32_t> ktab((size_t)head[1]), flags((size_t)head[2]), queries(3 * (size_t)head[3]);
        if (!read_all(in, ops.data(), ops.size() * sizeof(salve_resnet_op_t)) || !read_all(in, ktab.data(), ktab.size() * 4) ||
            !read_all(in, flags.data(), flags.size() * 4) || !read_all(in, queries.data(), queries.size() * 4))
            return 2;
        for (int32_t f : flags) {
            g_message = "";
            const std::vector<Step> plan = plan_resnet(ops.data(), (int)ops.size(), ktab.data(), ktab.size(), f);
            printf("P %d F %d:", p, f);
            if (plan.empty()) printf(" REFUSED %s", g_message);
            for (const Step& st : plan) printf(" %s", token(st).c_str());
            printf("\n");
        }
        for (size_t q = 0; q < queries.size(); q += 3) {
            const int32_t f = queries[q], op = queries[q + 1], batch = queries[q + 2];
            int answer = -1;
            for (const Step& st : plan_resnet(ops.data(), (int)ops.size(), ktab.data(), ktab.size(), f))
                if (st.first == op && st.kind == CONV) answer = conv_runs_wide(st, ops[(size_t)op], batch) ? 1 : 0;
            printf("Q %d %d %d %d: %d\n", p, f, op, batch, answer);
        }
    }
    fclose(in);
    return 0;
}
