"""The edit alignment of include/ds2hip.h (ds2_edit_align_i32), restated in plain Python: the full DP table, the traceback with its
tie rule, the counts and the two maps.  Nothing else."""


def align(a, b):
    """a: hypothesis, b: reference (sequences of comparable symbols) -> ((hits, subs, dels, ins), a_map, b_map)."""
    m, n = len(a), len(b)
    D = [[0] * (n + 1) for _ in range(m + 1)]
    for i in range(m + 1):
        D[i][0] = i
    for j in range(n + 1):
        D[0][j] = j
    for i in range(1, m + 1):
        for j in range(1, n + 1):
            D[i][j] = min(D[i - 1][j - 1] + (a[i - 1] != b[j - 1]), D[i][j - 1] + 1, D[i - 1][j] + 1)
    hits = subs = dels = ins = 0
    a_map, b_map = [-1] * m, [-1] * n
    i, j = m, n
    while i > 0 or j > 0:
        if i > 0 and j > 0 and D[i - 1][j - 1] + (a[i - 1] != b[j - 1]) == D[i][j]:
            a_map[i - 1], b_map[j - 1] = j - 1, i - 1
            if a[i - 1] == b[j - 1]:
                hits += 1
            else:
                subs += 1
            i, j = i - 1, j - 1
        elif j > 0 and D[i][j - 1] + 1 == D[i][j]:
            dels += 1
            j -= 1
        else:
            ins += 1
            i -= 1
    return (hits, subs, dels, ins), a_map, b_map


def align_padded(pairs, max_len):
    """The kernel's output arrays for a list of (a, b) pairs: counts (P,4), a_map and b_map (P,max_len) as nested lists, rows padded
    with -1."""
    counts, a_maps, b_maps = [], [], []
    for a, b in pairs:
        c, am, bm = align(a, b)
        counts.append(list(c))
        a_maps.append(am + [-1] * (max_len - len(am)))
        b_maps.append(bm + [-1] * (max_len - len(bm)))
    return counts, a_maps, b_maps
