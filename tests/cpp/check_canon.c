/* check_canon.c — the canonical-form switch of a plain-C checker object with float forms (resize_check.c, gaussian_blur_check.c and
 * linear_blur_check.c in one object; wavelet, fft, linear_algebra, resnet50 in one each): tests/checker_lib.py links a copy into each.  o_canon_fma is the form that
 * oracle/oracle_common.h's helpers read; the object is linked with -Wl,-Bsymbolic, so it is this definition and not
 * liboracle.so's that the checkers see when both are loaded. */
int o_canon_fma = 1;
void ck_set_canon(int fma) { o_canon_fma = fma != 0; }
int ck_get_canon(void) { return o_canon_fma; }
