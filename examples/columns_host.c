/* columns_host.c -- the host half of the metadata columns (rmu_columns_create / append / size / compact / set_option / free and the argument
 * checks of rmu_columns_select, all of which return before any HIP call) from a plain C program with its own main: no GPU is needed.
 * `make asan-columns` builds it with AddressSanitizer + UBSan against librmu_asan.so (the library's host code under the same sanitizers)
 * and runs it. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "rmu.h"

#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s (%s)\n", __LINE__, #c, rmu_last_error()); return 1; } } while (0)

int main(void) {
    rmu_columns_t* c = NULL;
    CHECK(rmu_columns_create(&c, 2, 16) == 0);
    enum { N = 5000 };
    int32_t* codes = malloc(sizeof(int32_t) * N * 2);
    for (int i = 0; i < N; ++i) { codes[2 * i] = i % 7; codes[2 * i + 1] = i % 300; }
    int64_t first = -1, n = 0, after = 0;
    int nf = 0;
    CHECK(rmu_columns_append(c, codes, 1000, &first) == 0 && first == 0);
    CHECK(rmu_columns_append(c, codes + 2000, N - 1000, &first) == 0 && first == 1000);
    codes[7] = -1;
    CHECK(rmu_columns_append(c, codes, 10, &first) == -1);
    codes[7] = 3 % 300;
    CHECK(rmu_columns_size(c, &n, &nf) == 0 && n == N && nf == 2);
    int64_t* map = malloc(sizeof(int64_t) * (N + 3));
    int64_t live = 0;
    for (int i = 0; i < N; ++i) map[i] = (i % 5 == 0) ? -1 : live++;
    map[N] = map[N + 1] = map[N + 2] = -1;
    CHECK(rmu_columns_compact(c, map, N - 1, &after) == -1);
    CHECK(rmu_columns_compact(c, map, N + 3, &after) == 0 && after == live);
    CHECK(rmu_columns_append(c, codes, 100, &first) == 0 && first == live);
    /* validation: every one of these returns before any HIP call */
    rmu_col_term terms[6] = {{0, 0, 1}, {1, 1, 4}, {0, 0, 1}, {0, 0, 1}, {0, 0, 1}, {0, 0, 1}};
    int32_t cs[1100];
    for (int i = 0; i < 1100; ++i) cs[i] = i;
    int32_t ptr2[3] = {0, 1, 2}, ptr6[2] = {0, 6};
    int64_t lp[3];
    cs[2] = 9; cs[3] = 7;
    CHECK(rmu_columns_select(c, terms, 2, cs, ptr2, 2, 0, NULL, 0, lp, 0) == -1 && strstr(rmu_last_error(), "selection 1"));
    cs[2] = 2; cs[3] = 3;
    terms[1].field = 2;
    CHECK(rmu_columns_select(c, terms, 2, cs, ptr2, 2, 0, NULL, 0, lp, 0) == -1 && strstr(rmu_last_error(), "selection 1"));
    terms[1].field = 1; terms[1].codes_end = 1027;
    CHECK(rmu_columns_select(c, terms, 2, cs, ptr2, 2, 0, NULL, 0, lp, 0) == -1 && strstr(rmu_last_error(), "1024"));
    terms[1].codes_end = 4;
    CHECK(rmu_columns_select(c, terms, 6, cs, ptr6, 1, 0, NULL, 0, lp, 0) == -1 && strstr(rmu_last_error(), "selection 0"));
    CHECK(rmu_columns_select(c, terms, 2, cs, ptr2, 0, 0, NULL, 0, lp, 0) == -1);
    CHECK(rmu_columns_set_option(c, RMU_COLUMNS_OPT_TILE_ROWS, 100) == -1 && rmu_columns_set_option(c, RMU_COLUMNS_OPT_TILE_ROWS, 64) == 0);
    CHECK(rmu_columns_free(c) == 0);
    free(codes); free(map);
    printf("columns host half: OK\n");
    return 0;
}
