// surfplan_cases.cpp — x265_amd/csrc/surfplan.h on its own (tests/test_surfplan.py): one case per line of standard input, one line of results each.
//   trim <cus> <cols> <n> <take arriving>...      -> the n trimmed takes
//   wide <freeCUs> <cap> <total>                  -> groups
//   grid <jobs1> <jobs2> <jobs3>                  -> waves, grid of the first sub-pel form (jobs: prefix sums)
//   ldsgrid <blocks1> <blocks2> <blocks3>         -> groups, grid of the second form
//   rows <rowsBuilt> <ctuRows> <S> <uploaded> <marginY> <picH>   -> rows possible
#include "surfplan.h"
#include <cstdio>
#include <cstring>
#include <vector>

struct Item { int take; bool arriving; };

int main()
{
    char what[16];
    while (scanf("%15s", what) == 1)
    {
        if (!strcmp(what, "trim"))
        {
            int cus, cols, n;
            if (scanf("%d %d %d", &cus, &cols, &n) != 3 || n < 0) return 2;
            std::vector<Item> items(n);
            for (Item& it : items)
            {
                int arriving;
                if (scanf("%d %d", &it.take, &arriving) != 2) return 2;
                it.arriving = arriving != 0;
            }
            xh::plan::trim_to_rounds(items.data(), n, cols, cus);
            for (int k = 0; k < n; k++) printf("%s%d", k ? " " : "", items[k].take);
            printf("\n");
        }
        else if (!strcmp(what, "wide"))
        {
            int freeCUs, cap, total;
            if (scanf("%d %d %d", &freeCUs, &cap, &total) != 3) return 2;
            printf("%d\n", xh::plan::wide_groups(freeCUs, cap, total));
        }
        else if (!strcmp(what, "grid"))
        {
            int jobs[4] = { 0, 0, 0, 0 };
            if (scanf("%d %d %d", &jobs[1], &jobs[2], &jobs[3]) != 3) return 2;
            const int waves = xh::plan::subpel_waves(jobs);
            printf("%d %d\n", waves, xh::plan::subpel_grid(waves));
        }
        else if (!strcmp(what, "ldsgrid"))
        {
            int b1, b2, b3;
            if (scanf("%d %d %d", &b1, &b2, &b3) != 3) return 2;
            const int groups = xh::plan::subpel_lds_groups(b1, b2, b3);
            printf("%d %d\n", groups, xh::plan::subpel_lds_grid(groups));
        }
        else if (!strcmp(what, "rows"))
        {
            int rowsBuilt, ctuRows, S, uploaded, marginY, picH;
            if (scanf("%d %d %d %d %d %d", &rowsBuilt, &ctuRows, &S, &uploaded, &marginY, &picH) != 6) return 2;
            printf("%d\n", xh::plan::rows_possible(rowsBuilt, ctuRows, S, uploaded, marginY, picH));
        }
        else
            return 2;
    }
    return 0;
}
