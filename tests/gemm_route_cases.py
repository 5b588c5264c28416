"""The fixed list of GEMM calls whose routing tests/gemm_routes.json records, and the argument structs they turn into.

A call is (name, grouped, [problem, ...]); a problem is a dict with M, N, K and, where they differ from the plain
contiguous product, ta (A outer-contiguous), bt (B reduce-contiguous), s (split_k), a_act / b_act / a_drop / b_drop
(operand transforms), A2 / B2 (addend operands), colsum, lda / ldb, a_off / b_off (operand pointers moved by that many
floats: alignment).  Pointers are made-up addresses: the plan query reads them for null-ness and alignment only.

The list holds the products of one C3a training step (the grouped calls of its plan log, every member of them as a call
of its own as well), both sides of every threshold of the routing rules, the operand and alignment variants, and grouped
calls of every kind of membership.  tests/test_gemm_routes_cpu.py holds mesm_gemm_plan to the recorded routes.
"""
import re

SWITCH_BF16X = (0, 2, 6)
SWITCH_TILE = (0, 1, 2, 3, 4, 6, 32, 64, 128)

# the grouped calls of one C3a step, as MESM_GEMM_PLAN_LOG prints them (first letter T: A outer-contiguous, second
# letter T: B reduce-contiguous, /s: split_k); the weight-gradient forms (TN) carry the bias gradient as colsum
STEP_CALLS = """
320x256x256NN/s1 256x256x320TN/s2
512x256x2400TN/s4 2400x256x512NN/s1 640x256x512NN/s1 32x256x256NN/s1 256x256x1024TN/s4 1024x256x256NN/s1 256x256x640TN/s4 256x256x640TN/s4 256x256x32TN/s1
512x256x2048TN/s3 256x256x4800TN/s8 512x256x2400TN/s4 2048x256x512NN/s1 2400x256x512NN/s1 4800x256x256NN/s1 32x256x256NN/s1 256x256x32TN/s1
32x256x256NT/s1 2400x512x256NT/s1 1024x256x256NT/s1 640x256x256NT/s1 640x256x256NT/s1
512x256x4864TN/s8 256x256x4864TN/s8 4864x256x512NN/s1 4864x256x256NN/s1
512x256x2112TN/s3 256x256x4800TN/s8 2112x256x512NN/s1 4800x256x256NN/s1
4800x256x256NT/s1 2048x512x256NT/s1 32x256x256NT/s1 2400x512x256NT/s1
32x256x256NN/s1 256x256x1024TN/s4 1024x256x256NN/s1 256x256x32TN/s1
32x1024x256NN/s1 256x1024x1024TN/s4 1024x1024x256NN/s1 256x1024x32TN/s1
320x256x256NN/s1 320x256x256NN/s1 256x256x320TN/s2 256x256x320TN/s2
256x256x4800TN/s8 4800x256x256NN/s1 32x256x256NN/s1 256x256x32TN/s1
256x1024x4800TN/s4 4800x1024x256NN/s1 32x1024x256NN/s1 256x1024x32TN/s1
2400x512x256NT/s1 2400x256x256NT/s1 320x256x256NT/s1
4864x512x256NT/s1 4864x256x256NT/s1
4800x256x256NT/s1 32x256x256NT/s1
4800x1024x256NT/s1 32x1024x256NT/s1
32x256x256NT/s1 1024x256x256NT/s1
32x1024x256NT/s1 1024x1024x256NT/s1
320x1024x256NN/s1 256x1024x320TN/s2
256x256x4864TN/s8 4864x256x256NN/s1
256x1024x4864TN/s4 4864x1024x256NN/s1
256x1024x4800TN/s4 4800x1024x256NN/s1
512x256x2400TN/s4 256x256x2400TN/s4 256x256x2400TN/s4 2400x256x512NN/s1 320x256x256NN/s1 256x256x320TN/s2
320x256x256NN/s1 320x256x256NN/s1 320x256x256NN/s1 256x256x320TN/s2 256x256x320TN/s2 256x256x320TN/s2
256x256x4800TN/s8 640x256x256NN/s1 4800x256x256NN/s1 64x256x256NN/s1 256x256x640TN/s4 256x256x64TN/s1
2400x256x2818NT/s1 2400x256x2818NT/s1 1024x256x512NT/s1 32x256x512NT/s1 1x256x512NT/s1 1x256x512NT/s1
2400x256x256NT/s1 1024x256x256NT/s1 2400x256x256NT/s1 32x256x256NT/s1 1x256x256NT/s1 1x256x256NT/s1
512x256x2400TN/s4 256x256x2400TN/s4 2400x256x512NN/s1 320x256x256NN/s1 256x256x320TN/s2
1024x256x4800TN/s4 4096x256x1024NN/s1 704x256x1024NN/s4 32x256x1024NN/s4 1024x256x32TN/s1
1024x256x4800TN/s4 4096x256x1024NN/s1 704x256x1024NN/s1 32x256x1024NN/s1 1024x256x32TN/s1
640x2x256NT/s1 640x256x256NT/s1 4800x256x256NT/s1 64x256x256NT/s1
4800x256x256NT/s1 2112x512x256NT/s1 1024x5003x256NT/s1 32x256x256NT/s1
32x256x1024NN/s4 1024x256x1024TN/s4 1024x256x1024NN/s4 1024x256x32TN/s1
32x256x1024NN/s1 1024x256x1024NN/s1 1024x256x1024TN/s4 1024x256x32TN/s1
320x512x256NT/s1 320x256x256NT/s1 320x256x256NT/s1 320x256x256NT/s1
320x256x768NN/s1 320x256x512NN/s1 768x256x320TN/s2 512x256x320TN/s2
4096x256x1024NT/s1 704x256x1024NT/s4 32x256x1024NT/s4
4096x256x1024NT/s1 704x256x1024NT/s1 32x256x1024NT/s1
320x512x256NT/s1 320x256x256NT/s1 320x256x256NT/s1
320x256x512NN/s1 768x256x320TN/s2 512x256x320TN/s2
320x256x256NT/s1 320x256x256NT/s1 320x256x256NT/s1
320x256x256NT/s1 320x1x256NT/s1 320x256x256NT/s1
320x256x256NN/s1 256x256x320TN/s2 256x256x320TN/s2
1024x256x4864TN/s4 4096x256x1024NN/s1 768x256x1024NN/s4
1024x256x4864TN/s4 4096x256x1024NN/s1 768x256x1024NN/s1
1024x256x4800TN/s4 4096x256x1024NN/s1 704x256x1024NN/s4
1024x256x4800TN/s4 4096x256x1024NN/s1 704x256x1024NN/s1
640x256x256NN/s1 256x256x640TN/s4
4800x256x256NT/s1 2112x512x256NT/s1
4096x256x1024NT/s1 768x256x1024NT/s4
4096x256x1024NT/s1 768x256x1024NT/s1
4096x256x1024NT/s1 704x256x1024NT/s4
4096x256x1024NT/s1 704x256x1024NT/s1
32x256x1024NT/s4 1024x256x1024NT/s4
32x256x1024NT/s1 1024x256x1024NT/s1
320x256x256NT/s1 320x256x256NT/s1
320x256x256NT/s1 320x1x256NT/s1
320x256x1024NN/s4 1024x256x320TN/s2
320x256x1024NN/s1 1024x256x320TN/s2
256x256x4800TN/s8 4800x256x256NN/s1
256x256x1024TN/s4 1024x256x256NN/s1
256x2818x2400TN/s4 256x2818x2400TN/s4 256x512x1024TN/s2 2400x2818x256NN/s1 1024x512x256NN/s1 2400x2818x256NN/s1 32x512x256NN/s1 1x512x256NN/s1 1x512x256NN/s1 256x512x32TN/s1 256x512x1TN/s1 256x512x1TN/s1
256x256x2400TN/s4 256x256x2400TN/s4 2400x256x256NN/s1 256x256x1024TN/s4 1024x256x256NN/s1 2400x256x256NN/s1 32x256x256NN/s1 1x256x256NN/s1 1x256x256NN/s1 256x256x32TN/s1 256x256x1TN/s1 256x256x1TN/s1
1024x256x5003NN/s4 256x256x4800TN/s8 5003x256x1024TN/s2 4800x256x256NN/s1
1024x256x5003NN/s1 256x256x4800TN/s8 5003x256x1024TN/s2 4800x256x256NN/s1
"""

ACT_RELU = 1


def _parse(tok):
    m = re.fullmatch(r"(\d+)x(\d+)x(\d+)([NT])([NT])/s(\d+)", tok)
    M, N, K, a, b, s = m.groups()
    p = dict(M=int(M), N=int(N), K=int(K), ta=a == "T", bt=b == "T", s=int(s))
    if p["ta"] and not p["bt"]:
        p["colsum"] = True
    return p


def P(M, N, K, **kw):
    return dict(M=M, N=N, K=K, **kw)


def calls():
    out = []

    def add(name, problems, grouped=True):
        out.append((name, grouped, problems))

    # -- the step's products: its grouped calls, then every distinct member alone
    step = [[_parse(t) for t in line.split()] for line in STEP_CALLS.strip().splitlines()]
    seen = []
    for i, c in enumerate(step):
        add("step call %d" % i, c)
        for p in c:
            if p not in seen:
                seen.append(p)
    for p in seen:
        add("step single %dx%dx%d" % (p["M"], p["N"], p["K"]), [p], grouped=False)

    # -- both sides of b64 = 128, 256/257, 512 and kper = 128, with M / K either side of 1024 and 2400, split and not;
    #    each alone, and beside a small product the 32 x 32 group takes (the grouped rules see the same thresholds)
    small = P(320, 256, 256, bt=True)
    tiles = [(64, 8128), (8128, 64), (1024, 512), (8192, 64), (1024, 1024), (4096, 256), (64, 16448), (16448, 64),
             (448, 4672), (4672, 448), (2048, 1024), (1024, 2048), (2399, 256), (2400, 256), (512, 1024), (1023, 512)]
    for M, N in tiles:
        for K in (256, 508, 512, 1023, 1024, 2399, 2400):
            for s in (1, 4):
                if s > 1 and K < 1023:
                    continue
                for bt in (True, False):
                    p = P(M, N, K, bt=bt, s=s)
                    add("threshold %dx%dx%d/s%d" % (M, N, K, s), [p], grouped=False)
                    if bt:
                        add("threshold pair %dx%dx%d/s%d" % (M, N, K, s), [p, small])
    # b64 = 127 / 128 and 511 / 512 through the split factor alone
    for M, N, K, s in ((2048, 256, 2400, 4), (2048, 256, 2400, 3), (2048, 1024, 4800, 1), (2048, 1022, 4800, 2)):
        add("split b64 %dx%dx%d/s%d" % (M, N, K, s), [P(M, N, K, ta=True, s=s, colsum=True)], grouped=False)

    # -- the tall tile: t96 = 159 / 160 and 256 / 257 at K = 511 / 512, with and without colsum, split and not
    for M, N in ((5088, 96), (1920, 256), (3072, 256), (96, 8224), (24672, 32), (2400, 256)):
        for K in (511, 512):
            for colsum in (False, True):
                for s in (1, 2):
                    p = P(M, N, K, bt=True, s=s, colsum=colsum)
                    add("tall %dx%dx%d" % (M, N, K), [p], grouped=False)
                    add("tall pair %dx%dx%d" % (M, N, K), [small, p])

    # -- 2 M N K either side of 1.5e9 beside a product of the 32 x 32 group (the mid-size rule of exact-f32 mode)
    for K in (1220, 1221):
        add("mid flops K=%d" % K, [P(2400, 256, K, bt=True), small])
        add("mid flops K=%d, no plain member" % K, [P(2400, 256, K, bt=True), P(2400, 256, K)])

    # -- operand transforms, each alone and in grouped calls (they force the all-layout kernel and keep a product out of
    #    the split-mode 64 x 64 group)
    for xf in (dict(a_act=ACT_RELU), dict(b_act=ACT_RELU), dict(a_drop=0.1), dict(b_drop=0.1)):
        for M, N, K in ((320, 256, 256), (2400, 256, 256), (2400, 256, 512), (4800, 256, 1024), (4800, 1024, 256), (256, 256, 4800)):
            for bt in (True, False):
                p = P(M, N, K, bt=bt, **xf)
                add("transform %dx%dx%d" % (M, N, K), [p], grouped=False)
                add("transform pair %dx%dx%d" % (M, N, K), [p, small])
                add("transform beside a 64 x 64 member %dx%dx%d" % (M, N, K), [p, P(4800, 256, 1024, bt=True), small])
    add("transforms, single stage", [P(320, 256, 256, bt=True, a_act=ACT_RELU), small, small])
    add("transforms, split weight gradient", [P(256, 256, 4800, ta=True, s=8, colsum=True, b_drop=0.1), P(256, 256, 320, ta=True, s=2)],)

    # -- addend operands (never on the LDS-DMA kernels): frag below 512 tiles of 64 x 64, the register tiles above and
    #    where frag's 16-byte rule refuses (K % 4, alignment, leading dimension)
    for add2 in (dict(A2=True), dict(B2=True)):
        for M, N, K in ((320, 256, 256), (2400, 256, 256), (4800, 1024, 256), (8192, 1024, 256), (16384, 2048, 256),
                        (320, 256, 258), (4800, 1024, 258), (16384, 2048, 258)):
            for lay in (dict(bt=True), dict(), dict(ta=True), dict(ta=True, bt=True)):
                add("addend %dx%dx%d" % (M, N, K), [P(M, N, K, **lay, **add2)], grouped=False)
        add("addend in a grouped call", [P(320, 256, 256, bt=True, **add2), small, small])
        add("addend and operand transform", [P(320, 256, 256, bt=True, a_act=ACT_RELU, **add2)], grouped=False)
        add("addend and operand transform, large", [P(4800, 1024, 256, b_drop=0.1, **add2)], grouped=False)
        for off in (1, 2):
            add("addend, operands %d floats off" % off, [P(320, 256, 256, bt=True, a_off=off, b_off=off, **add2)], grouped=False)
        add("addend, odd leading dimension", [P(320, 256, 256, bt=True, lda=257, ldb=257, **add2)], grouped=False)
        add("addend, leading dimension 258", [P(320, 256, 256, bt=True, lda=258, ldb=258, **add2)], grouped=False)

    # -- K < 4 and an outer extent < 4 (the LDS-DMA kernels refuse), every vector width of the register tiles
    for M, N, K in ((320, 256, 2), (320, 256, 3), (8192, 1024, 2), (16384, 2048, 2), (4800, 1024, 3)):
        for kw in (dict(bt=True), dict(), dict(ta=True), dict(bt=True, a_off=2, b_off=2), dict(bt=True, a_off=1),
                   dict(bt=True, lda=6, ldb=6), dict(bt=True, lda=5)):
            add("short reduce range %dx%dx%d" % (M, N, K), [P(M, N, K, **kw)], grouped=False)
    for kw in (dict(ta=True), dict(ta=True, bt=True), dict(ta=True, a_off=2), dict(ta=True, a_off=1)):
        for M in (2, 3, 4):
            add("outer extent %d" % M, [P(M, 256, 256, **kw)], grouped=False)
            add("outer extent %d, grouped" % M, [P(M, 256, 256, **kw), small])
    for N in (1, 2, 3, 4):
        add("outer extent N=%d" % N, [P(320, N, 256)], grouped=False)
        add("outer extent N=%d, reduce-contiguous" % N, [P(320, N, 256, bt=True)], grouped=False)
    add("odd outer extents", [P(321, 255, 256, ta=True)], grouped=False)
    add("odd outer extents, short K", [P(322, 254, 2, ta=True)], grouped=False)
    add("odd outer extents, short K, M % 4", [P(324, 253, 2, ta=True)], grouped=False)

    # -- grouped calls by membership
    big = P(4800, 256, 1024, bt=True)
    add("one member, 32 x 32", [small])
    add("one member, 64 x 64", [big])
    add("one member, tall", [P(2400, 256, 512, bt=True)])
    add("one member, alone", [P(320, 256, 256, bt=True, A2=True)])
    add("ten of the 32 x 32 class", [small] * 10)
    add("seventeen of the 32 x 32 class", [small] * 17)
    add("ten of the 64 x 64 class", [big] * 10)
    add("nine big, nine small, interleaved", [big, small] * 9)
    add("a tall member among small ones", [small, P(2400, 256, 512, bt=True), small])
    add("a tall member with colsum among small ones", [small, P(2400, 256, 512, bt=True, colsum=True), small])
    add("a member no grouped kernel takes", [small, P(320, 256, 256, bt=True, A2=True), big, P(320, 256, 2, bt=True)])
    for name, lays in (("NT", [dict(bt=True)]), ("NN", [dict()]), ("TN", [dict(ta=True)]), ("TT", [dict(ta=True, bt=True)]),
                       ("NN + TN", [dict(), dict(ta=True)]), ("NT + NN", [dict(bt=True), dict()]),
                       ("all four", [dict(bt=True), dict(), dict(ta=True), dict(ta=True, bt=True)])):
        add("layouts %s, 32 x 32" % name, [P(320, 256, 256, **l) for l in lays] * 2)
        add("layouts %s, 64 x 64" % name, [P(4800, 256, 1024, **l) for l in lays] * 2)
        add("layouts %s, two stages" % name, [P(4800, 256, 1024, **l) for l in lays] + [P(320, 256, 256, **l) for l in lays])
        add("layouts %s, ride-along" % name, [P(4800, 1024, 1024, **l) for l in lays] + [P(320, 256, 256, **l) for l in lays])
    add("longest reduce range first", [P(320, 256, 64, bt=True), P(320, 256, 512, bt=True), P(256, 256, 4800, ta=True, s=8),
                                      P(320, 256, 512), P(256, 256, 4800, ta=True, s=2)])
    return out


def make_args(problems):
    """(ctypes array of GemmArgs, n) for a list of problem dicts"""
    from mesm_amd import _lib
    arr = (_lib.GemmArgs * len(problems))()
    for i, p in enumerate(problems):
        g = arr[i]
        M, N, K = p["M"], p["N"], p["K"]
        ta, bt = p.get("ta", False), p.get("bt", False)
        g.M, g.N, g.K = M, N, K
        g.a_layout = _lib.LAYOUT_OUTER_CONTIG if ta else _lib.LAYOUT_REDUCE_CONTIG
        g.b_layout = _lib.LAYOUT_REDUCE_CONTIG if bt else _lib.LAYOUT_OUTER_CONTIG
        g.lda = p.get("lda", M if ta else K)
        g.ldb = p.get("ldb", K if bt else N)
        g.ldc = N
        g.A = 0x100000000 + 4 * p.get("a_off", 0)
        g.B = 0x200000000 + 4 * p.get("b_off", 0)
        g.C = 0x300000000 + 16 * i
        if p.get("A2"):
            g.A2 = 0x400000000 + 4 * p.get("a_off", 0)
        if p.get("B2"):
            g.B2 = 0x500000000 + 4 * p.get("b_off", 0)
        if p.get("colsum"):
            g.colsum = 0x600000000
        g.a_act, g.b_act = p.get("a_act", 0), p.get("b_act", 0)
        g.a_drop_p, g.b_drop_p = p.get("a_drop", 0.0), p.get("b_drop", 0.0)
        g.split_k = p.get("s", 1)
        g.out_scale = 1.0
    return arr, len(problems)


def member_index(c_pointer):
    return (c_pointer - 0x300000000) // 16
