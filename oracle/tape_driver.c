/* Driver of the tape-dispatch recorder (oracle/Makefile: _build/tape_dispatch) - TEST INFRASTRUCTURE.
 * Reads raw wire vectors from stdin, one uz_op per line: code, i[15], f[4], n, p[12] (floats in any strtod form, pointers as integers).
 * Runs each as a one-op tape on stream 0x99 through csrc/tape.hip, whose entry points are the recording stand-ins of tape_stubs.py,
 * and closes its record with "rc <return code>[ <uz_last_error()>]".  No HIP call is made and no device is opened. */
#include <stdio.h>
#include <string.h>
#include "uz_api.h"

int main(void) {
  for (;;) {
    uz_op op;
    long long n, p;
    memset(&op, 0, sizeof(op));
    if (scanf("%d", &op.code) != 1) return 0;
    for (int k = 0; k < 15; ++k) if (scanf("%d", &op.i[k]) != 1) return 2;
    for (int k = 0; k < 4; ++k) if (scanf("%f", &op.f[k]) != 1) return 2;
    if (scanf("%lld", &n) != 1) return 2;
    op.n = n;
    for (int k = 0; k < 12; ++k) { if (scanf("%lld", &p) != 1) return 2; op.p[k] = (void*)(uintptr_t)p; }
    const int rc = uz_run_tape(&op, 1, (void*)(uintptr_t)0x99);
    if (rc) printf("rc %d %s\n", rc, uz_last_error()); else printf("rc 0\n");
  }
}
