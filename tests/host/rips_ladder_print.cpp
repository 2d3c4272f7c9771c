// Prints the launch sequences of csrc/rips_ladder.h for tests/test_rips_ladder_model.py, one line per case and policy:
//     <flavour> <setting ...> <policy>: F<cap> R<cap> ... T
// dm: "dm <small|large> <fit flags of 1, 2, 4, 8 words> <words>", eeg: "eeg <words>", cloud: "cloud <words> <fits128>".
#include <stdio.h>
#include "rips_ladder.h"

using namespace rips_ladder;

static const char* const POLICY[5] = {"AUTO", "FIRST_PASS", "ONLY", "ONE_STEP", "LAST_RUNG"};

static void print_plans(const char* label, const Rungs& r)
{
    for (int policy = AUTO; policy <= LAST_RUNG; ++policy) {
        const Plan p = plan(policy, r);
        printf("%s %s:", label, POLICY[policy]);
        for (int i = 0; i < p.n; ++i) printf(" %c%d", p.step[i].retry ? 'R' : 'F', p.step[i].cap);
        if (p.last) printf(" T");
        printf("\n");
    }
}

int main()
{
    char label[64];
    const int dm_words[4] = {0, 1, 2, 4};
    for (int small = 1; small >= 0; --small)
        for (int nfit = 1; nfit <= 4; ++nfit) {          // the layouts grow with the capacity: the rungs that fit are the first nfit
            bool fits[4];
            for (int i = 0; i < 4; ++i) fits[i] = i < nfit;
            for (int w = 0; w < 4; ++w) {
                snprintf(label, sizeof label, "dm %s %d%d%d%d %d", small ? "small" : "large", fits[0], fits[1], fits[2],
                         fits[3], dm_words[w]);
                print_plans(label, dm_rungs(dm_words[w], small != 0, fits));
            }
        }
    for (int w = 0; w < 4; ++w) {
        snprintf(label, sizeof label, "eeg %d", dm_words[w]);
        print_plans(label, eeg_rungs(dm_words[w]));
    }
    for (int words = 1; words <= 2; ++words)
        for (int fits128 = 1; fits128 >= 0; --fits128) {
            snprintf(label, sizeof label, "cloud %d %d", words, fits128);
            print_plans(label, cloud_rungs(words, fits128 != 0));
        }
    return 0;
}
