// capacity_policy.cpp — the capacity and growth policy (node-replication_amd/csrc/capacity.hpp)
// without a GPU: a stand-alone program, built with the host compiler and
// -fsanitize=address,undefined and run by tests/test_capacity_policy.py. Exit status 0: every
// check held; else the failed checks are on stderr.
#include <stdint.h>
#include <stdio.h>

#include <initializer_list>

#include "../node-replication_amd/csrc/capacity.hpp"

using namespace nrg;

static int failures = 0;

#define CHECK(x)                                                        \
    do {                                                                \
        if (!(x)) {                                                     \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x);     \
            failures++;                                                 \
        }                                                               \
    } while (0)

constexpr uint64_t CAP = 64;

int main() {
    {  // fixed: no bound, so every chunk "fits" and nothing is accounted
        Growth g;
        for (uint64_t n : {1ull, 64ull, 65ull, 1ull << 40}) {
            CHECK(growth_fits(g, CAP, n));
            CHECK(g.len_ub == 0 && g.max_items == 0);
        }
    }
    {  // at the bound: the same
        Growth g{CAP, 7};
        for (uint64_t n : {1ull, 64ull, 65ull, 1ull << 40}) {
            CHECK(growth_fits(g, CAP, n));
            CHECK(g.len_ub == 7 && g.max_items == CAP);
        }
    }
    {  // accumulation: three chunks of 20 fit, the fourth asks for a re-read
        Growth g{4096, 0};
        for (uint64_t want : {20ull, 40ull, 60ull}) {
            CHECK(growth_fits(g, CAP, 20));
            CHECK(g.len_ub == want);
        }
        CHECK(!growth_fits(g, CAP, 20));
        CHECK(g.len_ub == 60);  // (the slow half accounts, after the exact read)
        // exact = 10: the balanced stream that never reallocates; the caller sets len_ub = exact + n
        CHECK(growth_target(g, CAP, 10 + 20) == CAP);
        g.len_ub = 10 + 20;
        CHECK(growth_fits(g, CAP, 20) && g.len_ub == 50);
        // exact = 60: double
        CHECK(growth_target(g, CAP, 60 + 20) == 128);
    }
    {  // need beyond double
        const Growth g{4096, 0};
        CHECK(growth_target(g, CAP, 300) == 300);
        CHECK(growth_target(g, CAP, 128) == 128 && growth_target(g, CAP, 129) == 129);
        CHECK(growth_target(g, CAP, 64) == CAP && growth_target(g, CAP, 65) == 128);
    }
    {  // clipping to the bound; then the structure is a fixed one (the overflow is the kernel's to latch)
        Growth g{100, 90};
        CHECK(growth_target(g, CAP, 300) == 100);
        CHECK(growth_target(g, CAP, 65) == 100);
        CHECK(growth_fits(g, 100, 300));
        CHECK(g.len_ub == 90);
    }
    {  // restore check
        CHECK(growth_admits(Growth{0, 0}, CAP, 64));
        CHECK(!growth_admits(Growth{0, 0}, CAP, 65));
        const Growth g{4096, 0};
        CHECK(growth_admits(g, CAP, 65));
        CHECK(growth_target(g, CAP, 65) == 128);
        CHECK(growth_admits(g, CAP, 4096));
        CHECK(!growth_admits(g, CAP, 4097));
        CHECK(growth_target(g, CAP, 4096) == 4096);
    }
    {  // limit values (nrg_set_max_capacity's arguments)
        const uint64_t st_limit = (1ull << 31) - 1, qu_limit = 1ull << 32;
        CHECK(!growth_bound_ok(63, CAP, st_limit));
        CHECK(!growth_bound_ok(1ull << 31, CAP, st_limit));
        CHECK(growth_bound_ok(st_limit, CAP, st_limit));
        CHECK(growth_bound_ok(64, CAP, st_limit));
        CHECK(growth_bound_ok(0, CAP, st_limit));
        CHECK(!growth_bound_ok(63, CAP, qu_limit));
        CHECK(growth_bound_ok(1ull << 32, CAP, qu_limit));
        CHECK(!growth_bound_ok((1ull << 32) + 1, CAP, qu_limit));
    }
    if (failures) fprintf(stderr, "capacity_policy: %d checks failed\n", failures);
    else printf("capacity_policy: ok\n");
    return failures ? 1 : 0;
}
