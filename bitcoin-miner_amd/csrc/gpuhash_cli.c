/* gpuhash_cli.c -- plain-C client of the C ABI (include/gpuhash.h), no Python/torch.
 *
 * It makes the same calls, in the same order, as the cgo binding in
 * integration/go/gpuhash/gpuhash.go.  That is the miner's sequence: open once, then per
 * Request (bitcoin/message.go:25-32) one gpuhash_min, answered as NewResult(hash, nonce)
 * (message.go:36-42), with the optional one-nonce self-check through gpuhash_hash_cpu
 * (== bitcoin.Hash, hash.go:11-15).
 *
 *   gpuhash_cli MSG LOWER UPPER        -> "Result <hash> <nonce>" (the client's output format)
 *   gpuhash_cli --range MSG LOWER COUNT -> one hash per line (gpuhash_hash_range)
 *   gpuhash_cli --below MSG LOWER UPPER TARGET -> "Result <hash> <nonce>" of the lowest nonce
 *                                         whose hash is <= TARGET, or "None" (gpuhash_first_below)
 *   gpuhash_cli --all-below MSG LOWER UPPER TARGET [CAP] -> "Total <n>", then one
 *                                         "Hit <hash> <nonce>" line for each of the lowest CAP
 *                                         (default GPUHASH_COLLECT_MAX) nonces whose hash is
 *                                         <= TARGET, ascending (gpuhash_collect_below)
 *   gpuhash_cli --batch FILE           -> FILE holds one job per line, "MSG LOWER UPPER" (MSG
 *                                         without blanks; empty lines are skipped); prints one
 *                                         "Result <hash> <nonce>" per job, in order, from ONE
 *                                         gpuhash_min_batch call ("-" reads standard input)
 *   gpuhash_cli --batch-below FILE     -> lines "MSG LOWER UPPER TARGET"; prints per job, in order,
 *                                         "Result <hash> <nonce>" of the lowest nonce whose hash is
 *                                         <= TARGET, or "None", from ONE gpuhash_first_below_batch call
 *   gpuhash_cli --batch-all-below FILE -> lines "MSG LOWER UPPER TARGET [CAP]"; prints per job, in order,
 *                                         "Total <n>" and then one "Hit <hash> <nonce>" line for each
 *                                         of the job's lowest CAP (default 256) nonces whose hash is
 *                                         <= TARGET, ascending, from ONE gpuhash_collect_below_batch call
 *   gpuhash_cli --version
 * --progress in front of any of the searches prints "<done> <total>" (gpuhash_progress) on stderr
 * about once a second, from a second thread.
 * --packed in front of --batch or --batch-all-below (after --progress, if both) sets
 * GPUHASH_LAYOUT_PACKED_ALWAYS: jobs of at most GPUHASH_PACKED_MAX_SPAN nonces run packed, for
 * files of tiny jobs.  The output is the same.
 * --early in front of --batch-below (after --progress) makes that one call
 * gpuhash_first_below_batch_early, for files of stamp jobs whose first hit lies early in a long
 * range: the front of every job runs packed, in doubling rounds.  The output is the same.
 * SIGINT and SIGTERM cancel the search in flight (gpuhash_cancel, from the handler): the run then
 * prints "Cancelled" on stderr, nothing on stdout, and exits 130.
 * Exit status: 0 ok, 2 usage, 3 library error (message on stderr), 4 self-check mismatch, 130 cancelled.
 */
#define _POSIX_C_SOURCE 200809L /* getline, strtok_r */
#include <inttypes.h>
#include <pthread.h>
#include <signal.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "gpuhash.h"

/* The context the signal handler cancels.  A signal that arrives before it is open is kept in
 * g_signalled and turned into the cancel as soon as it is (the latch then fails the first call). */
static gpuhash_ctx *volatile g_ctx;
static volatile sig_atomic_t g_signalled;
static int g_progress;
static int g_packed;
static int g_early;

static void on_signal(int sig) {
    (void)sig;
    g_signalled = 1;
    gpuhash_ctx *ctx = g_ctx;
    if (ctx) gpuhash_cancel(ctx); /* one atomic store: async-signal-safe */
}

static void *progress_main(void *arg) {
    (void)arg;
    for (;;) {
        struct timespec second = {1, 0};
        nanosleep(&second, NULL);
        uint64_t done = 0, total = 0;
        gpuhash_ctx *ctx = g_ctx;
        if (!ctx) return NULL;
        if (gpuhash_progress(ctx, &done, &total) == GPUHASH_OK && total)
            fprintf(stderr, "%" PRIu64 " %" PRIu64 "\n", done, total);
    }
}

static pthread_t g_progress_thread;

/* gpuhash_open for this program: the context becomes the signal handler's, and --progress's. */
static int open_ctx(gpuhash_ctx **out) {
    const int rc = gpuhash_open(NULL, 0, out);
    if (rc) return rc;
    g_ctx = *out;
    if (g_signalled) gpuhash_cancel(*out);
    if (g_packed) gpuhash_set_layout_policy(*out, GPUHASH_LAYOUT_AUTO | GPUHASH_LAYOUT_PACKED_ALWAYS);
    if (g_progress && pthread_create(&g_progress_thread, NULL, progress_main, NULL) != 0) g_progress = 0;
    return rc;
}

static void close_ctx(gpuhash_ctx *ctx) {
    signal(SIGINT, SIG_DFL); /* from here on a signal ends the program as it would any other */
    signal(SIGTERM, SIG_DFL);
    g_ctx = NULL; /* the handler and the progress thread stop using it */
    if (g_progress) {
        pthread_cancel(g_progress_thread); /* it is in nanosleep, or about to be */
        pthread_join(g_progress_thread, NULL);
    }
    gpuhash_close(ctx);
}

static int parse_u64(const char *s, uint64_t *out) {
    char *end = NULL;
    if (!s || !*s || *s == '-') return -1;
    unsigned long long v = strtoull(s, &end, 10);
    if (*end) return -1;
    *out = (uint64_t)v;
    return 0;
}

static int fail(const char *what, int rc) {
    if (rc == GPUHASH_ECANCELED) {
        fprintf(stderr, "Cancelled\n");
        return 130;
    }
    fprintf(stderr, "%s: %s (rc=%d)\n", what, gpuhash_strerror(rc), rc);
    return 3;
}

/* A --batch-all-below line without a CAP has room for this many hits: the output arrays hold the
 * sum of the jobs' rooms, and the batch is built for sparse hits. */
#define BATCH_ALL_DEFAULT_CAP 256

/* --batch-all-below, the jobs read: one gpuhash_collect_below_batch call, --all-below's self-check
 * per listed hit, and the output. */
static int batch_all_main(gpuhash_ctx *ctx, const uint8_t *msgs, const size_t *off, size_t njobs, const uint64_t *lower,
                          const uint64_t *upper, const uint64_t *target, const uint64_t *caps) {
    size_t *out_off = (size_t *)malloc((njobs + 1) * sizeof *out_off);
    uint64_t *totals = (uint64_t *)malloc(njobs * sizeof *totals);
    uint64_t *nonces = NULL, *hashes = NULL;
    int status = 0, oversized = 0;
    if (out_off && totals) {
        out_off[0] = 0;
        for (size_t k = 0; k < njobs; k++) { /* an oversized CAP is the library's argument error to report */
            oversized = oversized || caps[k] > GPUHASH_COLLECT_MAX;
            out_off[k + 1] = out_off[k] + (caps[k] > GPUHASH_COLLECT_MAX ? (size_t)GPUHASH_COLLECT_MAX + 1 : (size_t)caps[k]);
        }
        /* ... which it does before it touches the arrays, so only then are they short */
        const size_t room = oversized || !out_off[njobs] ? 1 : out_off[njobs];
        nonces = (uint64_t *)malloc(room * sizeof *nonces);
        hashes = (uint64_t *)malloc(room * sizeof *hashes);
    }
    if (!out_off || !totals || !nonces || !hashes) {
        fprintf(stderr, "out of memory\n");
        status = 3;
    } else {
        const int rc = gpuhash_collect_below_batch(ctx, msgs, off, njobs, lower, upper, target, out_off, nonces, hashes, totals);
        if (rc) status = fail("gpuhash_collect_below_batch", rc);
    }
    for (size_t k = 0; k < njobs && !status; k++) {
        const uint64_t held = totals[k] < caps[k] ? totals[k] : caps[k];
        for (uint64_t i = 0; i < held && !status; i++) {
            const uint64_t x = nonces[out_off[k] + i], h = hashes[out_off[k] + i];
            if (gpuhash_hash_cpu(msgs + off[k], off[k + 1] - off[k], x) != h || h > target[k] || x < lower[k] ||
                x > upper[k] || (i && x <= nonces[out_off[k] + i - 1])) {
                fprintf(stderr, "self-check failed at job %zu, hit %" PRIu64 " (nonce %" PRIu64 ")\n", k, i, x);
                status = 4;
            }
        }
    }
    for (size_t k = 0; k < njobs && !status; k++) {
        const uint64_t held = totals[k] < caps[k] ? totals[k] : caps[k];
        printf("Total %" PRIu64 "\n", totals[k]);
        for (uint64_t i = 0; i < held; i++)
            printf("Hit %" PRIu64 " %" PRIu64 "\n", hashes[out_off[k] + i], nonces[out_off[k] + i]);
    }
    free(out_off);
    free(totals);
    free(nonces);
    free(hashes);
    return status;
}

/* --batch: every job of the file in one gpuhash_min_batch call; --batch-below (below == 1): in
 * one gpuhash_first_below_batch call, each line with a TARGET; --batch-all-below (below == 2): in
 * one gpuhash_collect_below_batch call, each line with a TARGET and an optional CAP. */
static int batch_main(const char *path, int below) {
    FILE *f = strcmp(path, "-") == 0 ? stdin : fopen(path, "r");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path);
        return 2;
    }
    size_t njobs = 0, cap = 0, bytes = 0, bytes_cap = 0;
    uint8_t *msgs = NULL;
    size_t *off = NULL;
    uint64_t *lower = NULL, *upper = NULL, *target = NULL, *caps = NULL;
    char *line = NULL;
    size_t line_cap = 0;
    int status = 0;
    while (!status && getline(&line, &line_cap, f) >= 0) {
        char *save = NULL;
        const char *m = strtok_r(line, " \t\r\n", &save);
        if (!m) continue; /* an empty line */
        const char *lo = strtok_r(NULL, " \t\r\n", &save), *hi = strtok_r(NULL, " \t\r\n", &save);
        const char *tg = below ? strtok_r(NULL, " \t\r\n", &save) : NULL;
        const char *cp = below == 2 ? strtok_r(NULL, " \t\r\n", &save) : NULL;
        uint64_t a, b, t = 0, c = BATCH_ALL_DEFAULT_CAP;
        if (!lo || !hi || (below && (!tg || parse_u64(tg, &t))) || (cp && parse_u64(cp, &c)) ||
            strtok_r(NULL, " \t\r\n", &save) || parse_u64(lo, &a) || parse_u64(hi, &b)) {
            fprintf(stderr, "line %zu: expected MSG LOWER UPPER%s\n", njobs + 1,
                    below == 2 ? " TARGET [CAP]" : below ? " TARGET" : "");
            status = 2;
            break;
        }
        const size_t len = strlen(m);
        if (njobs == cap) {
            cap = cap ? 2 * cap : 64;
            off = (size_t *)realloc(off, (cap + 1) * sizeof *off);
            lower = (uint64_t *)realloc(lower, cap * sizeof *lower);
            upper = (uint64_t *)realloc(upper, cap * sizeof *upper);
            target = (uint64_t *)realloc(target, cap * sizeof *target);
            caps = (uint64_t *)realloc(caps, cap * sizeof *caps);
        }
        if (bytes + len + 1 > bytes_cap) {
            bytes_cap = 2 * (bytes + len + 1);
            msgs = (uint8_t *)realloc(msgs, bytes_cap);
        }
        if (!off || !lower || !upper || !target || !caps || !msgs) {
            fprintf(stderr, "out of memory\n");
            status = 3;
            break;
        }
        memcpy(msgs + bytes, m, len);
        off[njobs] = bytes;
        bytes += len;
        lower[njobs] = a;
        upper[njobs] = b;
        target[njobs] = t;
        caps[njobs] = c;
        off[++njobs] = bytes;
    }
    free(line);
    if (f != stdin) fclose(f);
    uint64_t *h = NULL, *n = NULL;
    int *found = NULL;
    if (!status && njobs == 0) {
        fprintf(stderr, "no jobs in %s\n", path);
        status = 2;
    }
    if (!status) {
        h = (uint64_t *)malloc(njobs * sizeof *h);
        n = (uint64_t *)malloc(njobs * sizeof *n);
        found = (int *)malloc(njobs * sizeof *found);
        gpuhash_ctx *ctx = NULL;
        int rc = h && n && found ? open_ctx(&ctx) : GPUHASH_ENOMEM;
        if (rc) {
            status = fail("gpuhash_open", rc);
        } else if (below == 2) {
            status = batch_all_main(ctx, msgs, off, njobs, lower, upper, target, caps);
            close_ctx(ctx);
        } else if (below) {
            rc = g_early ? gpuhash_first_below_batch_early(ctx, msgs, off, njobs, lower, upper, target, 0, 0, h, n, found)
                         : gpuhash_first_below_batch(ctx, msgs, off, njobs, lower, upper, target, h, n, found);
            if (rc) status = fail(g_early ? "gpuhash_first_below_batch_early" : "gpuhash_first_below_batch", rc);
            for (size_t k = 0; k < njobs && !status; k++) { /* --below's self-check, per found job */
                if (found[k] && (gpuhash_hash_cpu(msgs + off[k], off[k + 1] - off[k], n[k]) != h[k] || h[k] > target[k] ||
                                 n[k] < lower[k] || n[k] > upper[k])) {
                    fprintf(stderr, "self-check failed at job %zu: Hash(msg, %" PRIu64 ") != %" PRIu64
                                    " or above the target\n", k, n[k], h[k]);
                    status = 4;
                }
            }
            for (size_t k = 0; k < njobs && !status; k++) {
                if (found[k]) printf("Result %" PRIu64 " %" PRIu64 "\n", h[k], n[k]);
                else printf("None\n");
            }
            close_ctx(ctx);
        } else {
            rc = gpuhash_min_batch(ctx, msgs, off, njobs, lower, upper, h, n);
            if (rc) status = fail("gpuhash_min_batch", rc);
            for (size_t k = 0; k < njobs && !status; k++) {
                if (gpuhash_hash_cpu(msgs + off[k], off[k + 1] - off[k], n[k]) != h[k] || n[k] < lower[k] ||
                    n[k] > upper[k]) {
                    fprintf(stderr, "self-check failed at job %zu: Hash(msg, %" PRIu64 ") != %" PRIu64 "\n", k, n[k], h[k]);
                    status = 4;
                }
            }
            for (size_t k = 0; k < njobs && !status; k++) printf("Result %" PRIu64 " %" PRIu64 "\n", h[k], n[k]);
            close_ctx(ctx);
        }
    }
    free(h);
    free(n);
    free(found);
    free(target);
    free(caps);
    free(msgs);
    free(off);
    free(lower);
    free(upper);
    return status;
}

int main(int argc, char **argv) {
    struct sigaction sa;
    memset(&sa, 0, sizeof sa);
    sa.sa_handler = on_signal;
    sigemptyset(&sa.sa_mask);
    sigaction(SIGINT, &sa, NULL);
    sigaction(SIGTERM, &sa, NULL);
    if (argc >= 2 && strcmp(argv[1], "--progress") == 0) {
        g_progress = 1;
        argv[1] = argv[0];
        argv++;
        argc--;
    }
    if (argc >= 2 && strcmp(argv[1], "--packed") == 0) {
        g_packed = 1;
        argv[1] = argv[0];
        argv++;
        argc--;
    }
    if (argc == 4 && strcmp(argv[1], "--early") == 0 && strcmp(argv[2], "--batch-below") == 0) {
        g_early = 1;
        argv[1] = argv[0];
        argv++;
        argc--;
    }
    if (argc == 2 && strcmp(argv[1], "--version") == 0) {
        printf("%s\n", gpuhash_version());
        return 0;
    }
    if (argc == 3 && strcmp(argv[1], "--batch") == 0) return batch_main(argv[2], 0);
    if (argc == 3 && strcmp(argv[1], "--batch-below") == 0) return batch_main(argv[2], 1);
    if (argc == 3 && strcmp(argv[1], "--batch-all-below") == 0) return batch_main(argv[2], 2);
    const int range_mode = argc == 5 && strcmp(argv[1], "--range") == 0;
    const int below_mode = argc == 6 && strcmp(argv[1], "--below") == 0;
    const int all_mode = (argc == 6 || argc == 7) && strcmp(argv[1], "--all-below") == 0;
    if (!range_mode && !below_mode && !all_mode && argc != 4) {
        fprintf(stderr, "usage: %s MSG LOWER UPPER | --range MSG LOWER COUNT | --below MSG LOWER UPPER TARGET"
                        " | --all-below MSG LOWER UPPER TARGET [CAP] | [--packed] --batch FILE | [--early] --batch-below FILE | [--packed] --batch-all-below FILE | --version\n", argv[0]);
        return 2;
    }
    const int opt = range_mode || below_mode || all_mode;
    const char *msg = argv[opt ? 2 : 1];
    uint64_t a, b, target = 0, cap = GPUHASH_COLLECT_MAX;
    if (parse_u64(argv[opt ? 3 : 2], &a) || parse_u64(argv[opt ? 4 : 3], &b) ||
        ((below_mode || all_mode) && parse_u64(argv[5], &target)) || (argc == 7 && parse_u64(argv[6], &cap))) {
        fprintf(stderr, "bad number\n");
        return 2;
    }
    gpuhash_ctx *ctx = NULL;
    int rc = open_ctx(&ctx);
    if (rc) return fail("gpuhash_open", rc);
    const size_t len = strlen(msg);
    int status = 0;
    if (range_mode) {
        uint64_t *out = (uint64_t *)malloc((size_t)(b ? b : 1) * sizeof(uint64_t));
        if (!out) { close_ctx(ctx); return 3; }
        rc = gpuhash_hash_range(ctx, (const uint8_t *)msg, len, a, b, out);
        if (rc) status = fail("gpuhash_hash_range", rc);
        for (uint64_t i = 0; !rc && i < b; i++) printf("%" PRIu64 "\n", out[i]);
        free(out);
    } else if (below_mode) {
        uint64_t h = 0, n = 0;
        int found = 0;
        rc = gpuhash_first_below(ctx, (const uint8_t *)msg, len, a, b, target, &h, &n, &found);
        if (rc) {
            status = fail("gpuhash_first_below", rc);
        } else if (!found) {
            printf("None\n");
        } else if (gpuhash_hash_cpu((const uint8_t *)msg, len, n) != h || h > target) {
            fprintf(stderr, "self-check failed: Hash(msg, %" PRIu64 ") != %" PRIu64 " or above the target\n", n, h);
            status = 4;
        } else {
            printf("Result %" PRIu64 " %" PRIu64 "\n", h, n);
        }
    } else if (all_mode) {
        /* an oversized CAP is the library's argument error to report, so only the
         * allocation is clamped */
        const size_t room = cap > GPUHASH_COLLECT_MAX ? GPUHASH_COLLECT_MAX : (size_t)cap;
        uint64_t *nonces = (uint64_t *)malloc((room ? room : 1) * sizeof(uint64_t));
        uint64_t *hashes = (uint64_t *)malloc((room ? room : 1) * sizeof(uint64_t));
        uint64_t total = 0;
        if (!nonces || !hashes) { free(nonces); free(hashes); close_ctx(ctx); return 3; }
        rc = gpuhash_collect_below(ctx, (const uint8_t *)msg, len, a, b, target, nonces, hashes,
                                   cap > GPUHASH_COLLECT_MAX ? (size_t)GPUHASH_COLLECT_MAX + 1 : (size_t)cap, &total);
        if (rc) {
            status = fail("gpuhash_collect_below", rc);
        } else {
            const uint64_t k = total < cap ? total : cap;
            for (uint64_t i = 0; i < k && !status; i++) {
                if (gpuhash_hash_cpu((const uint8_t *)msg, len, nonces[i]) != hashes[i] || hashes[i] > target ||
                    (i && nonces[i] <= nonces[i - 1])) {
                    fprintf(stderr, "self-check failed at hit %" PRIu64 " (nonce %" PRIu64 ")\n", i, nonces[i]);
                    status = 4;
                }
            }
            if (!status) {
                printf("Total %" PRIu64 "\n", total);
                for (uint64_t i = 0; i < k; i++) printf("Hit %" PRIu64 " %" PRIu64 "\n", hashes[i], nonces[i]);
            }
        }
        free(nonces);
        free(hashes);
    } else {
        uint64_t h = 0, n = 0;
        rc = gpuhash_min(ctx, (const uint8_t *)msg, len, a, b, &h, &n);
        if (rc) {
            status = fail("gpuhash_min", rc);
        } else if (gpuhash_hash_cpu((const uint8_t *)msg, len, n) != h) {
            fprintf(stderr, "self-check failed: Hash(msg, %" PRIu64 ") != %" PRIu64 "\n", n, h);
            status = 4;
        } else {
            printf("Result %" PRIu64 " %" PRIu64 "\n", h, n);
        }
    }
    close_ctx(ctx);
    return status;
}
