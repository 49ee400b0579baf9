"""Host tests (no GPU, no library) of _lib.parse_header on synthetic header text: what it reads, and that it raises LidarHipError
naming the declaration for everything it would otherwise have to guess."""
import ctypes as C

import pytest

from lidardetection_amd._lib import LidarHipError, parse_header

vp, i32 = C.c_void_p, C.c_int

HEADER = """
/* a comment with parentheses: int lidar_in_comment(int a, float b); and (more) */
#ifndef LIDAR_HIP_H
#define LIDAR_HIP_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif
#define LIDAR_A_ZERO 0
#define LIDAR_A_MINUS (-4) /* a comment (with parentheses) behind a value */
#define LIDAR_A_SHIFT (1 << 20)
#define LIDAR_A_LONG 1ll << 22
#define LIDAR_A_HEX 0x7fffffffLL
#define LIDAR_A_SUM (2 + 3 * 4)      // 14: * binds tighter than +
#define LIDAR_A_SHIFTED_SUM 1 << 2 + 1
#define LIDAR_A_NEGATED -(3 + 1) * 2
#define LIDAR_FUNCTION_LIKE(x) ((x) + 1)
#define NOT_OURS 5
size_t lidar_bytes(int batch, long long rows);   // lidar_line_comment(int x);
void lidar_nothing(void *p);
void *lidar_make(void);
const void *lidar_peek(void *ws, int n);
float lidar_ms(void *timer);
long long lidar_plan(const long long *numel, double lr, float eps, size_t n);
int lidar_spread(const float *a,
                 float const *b, const float *const c,
                 void *const *d, unsigned char **e,
                 int
                 n);
int lidar_widths(unsigned flags, uint32_t mask, int64_t big, const int64_t *list, unsigned int u, unsigned char byte);
int lidar_unnamed(int, const float *, long long);
int lidar_twice(int a, float *out);
int lidar_twice(int other_name, float *const out);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_reads_every_declared_form():
    sigs, limits = parse_header(HEADER)
    assert sigs == {
        "lidar_bytes": (C.c_size_t, [i32, C.c_longlong]),
        "lidar_nothing": (None, [vp]),
        "lidar_make": (vp, []),
        "lidar_peek": (vp, [vp, i32]),
        "lidar_ms": (C.c_float, [vp]),
        "lidar_plan": (C.c_longlong, [vp, C.c_double, C.c_float, C.c_size_t]),
        "lidar_spread": (i32, [vp, vp, vp, vp, vp, i32]),
        "lidar_widths": (i32, [C.c_uint, C.c_uint32, C.c_int64, vp, C.c_uint, C.c_ubyte]),
        "lidar_unnamed": (i32, [i32, vp, C.c_longlong]),
        "lidar_twice": (i32, [i32, vp]),
    }
    assert limits == {"LIDAR_A_ZERO": 0, "LIDAR_A_MINUS": -4, "LIDAR_A_SHIFT": 1 << 20, "LIDAR_A_LONG": 1 << 22,
                      "LIDAR_A_HEX": 0x7fffffff, "LIDAR_A_SUM": 14, "LIDAR_A_SHIFTED_SUM": 8, "LIDAR_A_NEGATED": -8}


def test_empty_text_declares_nothing():
    assert parse_header("") == ({}, {}) and parse_header("/* int lidar_x(int a); */\n") == ({}, {})


@pytest.mark.parametrize("decl, names", [
    ("int lidar_bad(hipStream_t stream);", ["lidar_bad", "hipStream_t"]),                 # unknown base type, by value
    ("int lidar_bad(const my_box *boxes);", ["lidar_bad", "my_box"]),                     # ... and behind a pointer
    ("short lidar_bad(int a);", ["lidar_bad", "short"]),                                  # ... and as the return type
    ("int lidar_bad(struct box b);", ["lidar_bad", "struct"]),                            # a struct by value
    ("int lidar_bad(float range6[6]);", ["lidar_bad", "array"]),
    ("int lidar_bad(int n, void (*done)(int, int));", ["lidar_bad", "function-pointer"]),
    ("int lidar_bad(const char *fmt, ...);", ["lidar_bad", "variadic"]),
    ("int lidar_bad();", ["lidar_bad", "(void)"]),                                        # unspecified parameters in C
    ("int lidar_bad(void v);", ["lidar_bad", "void"]),
    ("int lidar_bad(int a b);", ["lidar_bad"]),
    ("int lidar_bad(int a, long long n);\nint lidar_bad(int a, int n);", ["lidar_bad", "twice"]),
    ("int lidar_bad(int a);\nfloat lidar_bad(int a);", ["lidar_bad", "twice"]),
    ("typedef struct { int a; } lidar_box;", []),                                         # not a function declaration at all
    ("#define LIDAR_BAD 1.5f", ["LIDAR_BAD"]),
    ("#define LIDAR_BAD (1 << 4", ["LIDAR_BAD"]),
    ("#define LIDAR_BAD 8 - 1", ["LIDAR_BAD"]),                                           # an operator outside the accepted set
    ("#define LIDAR_BAD LIDAR_OTHER", ["LIDAR_BAD"]),
    ("#define LIDAR_BAD 1\n#define LIDAR_BAD 2", ["LIDAR_BAD", "twice"]),
])
def test_refuses_what_it_would_have_to_guess(decl, names):
    with pytest.raises(LidarHipError) as e:
        parse_header("int lidar_fine(int a);\n" + decl + "\n")
    for n in names:
        assert n in str(e.value), str(e.value)
