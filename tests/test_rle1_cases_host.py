"""Every family of tests/rle1_cases.py contains what it says: asserted from the oracle's blocks and the plain per-byte model of
the chunk rule alone.  A family that misses its shape is a broken test.  CPU only; the GPU tests of the same families are
tests/test_gpu_rle1_cap.py and tests/test_gpu_rle1_batch.py."""
import numpy as np

import rle1_cases as rc


def _facts(oracle, key, data, cap):
    m = rc.model(key, data)
    f = rc.block_facts(m, rc.want(oracle, key, data, cap), cap)
    rc.check_model(f)
    return m, f


def test_model_is_the_oracle_on_single_runs(oracle):
    # one run of every length around the chunk rule's steps, as one block: emitted_fresh, the model's prefix and the oracle agree
    for L in list(range(1, 12)) + list(range(250, 265)) + list(range(505, 520)) + [1020, 5000]:
        d = rc.run(0x41, L)
        m = rc.Model(d)
        assert oracle.rle1_len(d) == int(m.G[-1]) == int(rc.emitted_fresh(L)), L
        assert rc.absorbed_flag(d) == ((L - 1) % 255 >= 4)
    assert rc.Model(rc.runfree(5000, 3)).G[-1] == 5000 and oracle.rle1_len(rc.runfree(5000, 3)) == 5000
    assert rc.Model(np.zeros(0, np.uint8)).n == 0


def test_family_a_boundary_phases(oracle):
    cases = rc.family_a()
    caps = {c for _, c in cases}
    assert caps >= set(range(rc.CAP_FLOOR, 13)) | set(range(254, 262)) | set(range(1274, 1282)) | set(range(4093, 4102))
    assert len({c for c in caps if c % 5 == 1}) >= 5 and {c % 5 for c in caps} == {0, 1, 2, 3, 4}
    tags, boundaries = set(), 0
    for name, cap in cases:
        data = rc.inputs()[name]
        assert 20000 <= data.size <= 70 * 1024, (name, data.size)
        m, f = _facts(oracle, name, data, cap)
        tags |= rc.boundary_tags(m, f)
        boundaries += len(f["S"])
    assert not rc.FAMILY_A_NEEDS - tags, "family A misses %s" % sorted(rc.FAMILY_A_NEEDS - tags)
    assert "unclean_by_probe" in tags
    assert boundaries > 50000
    # the planted runs are the lengths the family names, each one there
    m = rc.model("a_large", rc.inputs()["a_large"])
    assert set(rc.RUNLENS) <= set((m.re - m.rs)[m.head].tolist())
    # where the count byte is the block's last byte it is stored as 0
    data = rc.inputs()["a_small"]
    for cap in (5, 10):
        m, f = _facts(oracle, "a_small", data, cap)
        hit = np.nonzero(f["full"] & (f["dp_last"] == 3) & (f["emitted"] == cap) & f["cont"])[0]
        assert hit.size
        for k in hit[:20]:
            assert rc.want(oracle, "a_small", data, cap)[k][0][-1] == 0


def test_family_b_speculation_rounds(oracle):
    b = rc.family_b()
    data, cap = b["rounds"]
    m, f = _facts(oracle, "b_rounds", data, cap)
    clean = rc.clean_flags(m, f)
    first_bad = int(np.argmin(clean))
    assert first_bad >= 70 and first_bad >= 2 * rc.NSPEC + 6          # two whole rounds of 32 clean boundaries and more
    assert f["cont"][first_bad] and (m.re - m.rs)[f["E"][first_bad]] == 40      # the unclean one: the next block starts in the run of 40
    assert np.all(clean[first_bad + 1: first_bad + 1 + rc.NSPEC + 2])          # another whole round behind it
    for k in (31, 32, 33, 64):
        for x in (0, 1):
            data, cap = b["totals_%d_%d" % (k, x)]
            assert oracle.rle1_len(data) == k * cap + x
            assert len(rc.want(oracle, "b_totals_%d_%d" % (k, x), data, cap)) == k + x
    data, cap = b["dropped_count_at_eof"]
    m, f = _facts(oracle, "b_dropped", data, cap)
    assert oracle.rle1_len(data) == 33 * cap + 1 and len(f["S"]) == 33 and f["emitted"][-1] == cap + 1 and f["L"][-1] == cap


def test_family_c_geometry(oracle):
    c = rc.family_c(oracle.rle1_len)
    ends = set()
    for cap in rc.CAPS_255 + rc.CAPS_4096:
        data, cc = c["offsets_%d" % cap]
        m, f = _facts(oracle, "c_offsets", data, cc)
        assert np.array_equal(f["E"][:-1], cap * np.arange(1, len(f["E"])))
        ends |= set(f["E"][:-1].tolist())
    assert {e % 256 for e in ends} >= {255, 0, 1} and {e % 4096 for e in ends} >= {4095, 0, 1}
    assert {(e - 1) % 256 for e in ends} >= {255, 0, 1} and {(e - 1) % 4096 for e in ends} >= {4095, 0, 1}
    data, cap = c["long_run_start_inside"]
    m, f = _facts(oracle, "c_long", data, cap)
    s, r_end = int(f["S"][1]), int(f["r_end"][1])
    assert f["inrun"][1] and r_end - s > 2 * rc.RT and r_end // rc.RT >= s // rc.RT + 2
    assert not m.head[s + 1: (s // rc.RT + 1) * rc.RT].any()          # no run start behind s in its tile: r_end is next_bnd's
    data, cap = c["start_in_last_subtile"]
    m, f = _facts(oracle, "c_subtile", data, cap)
    s, r_end = int(f["S"][1]), int(f["r_end"][1])
    assert f["inrun"][1] and s % rc.RT >= rc.RT - 256 and r_end // rc.RT == s // rc.RT + 1
    assert rc.emitted_fresh(r_end - s) < cap                           # the walk goes on behind the run (base0 > 0)


def test_family_c_chunk_seam(oracle):
    seam = rc.SC * rc.RT
    assert rc.C_SEAM_CAP % 5 == 1 and 95000 < rc.C_SEAM_CAP < 105000
    for L in rc.C_SEAM_RUNS:
        data = rc.chunk_seam_input(L)
        assert data.size == 4 * 1024 * 1024 + 65536 and (data.size + rc.RT - 1) // rc.RT > rc.SC
        m = rc.model("c_seam_%d" % L, data)
        assert m.rs[seam] < seam < m.re[seam] and m.re[seam] - m.rs[seam] == L      # the run straddles the chunk seam
        # the carries across the seam are real data: tile 1024's run start lies in chunk 0, tile 1023's next run start in
        # chunk 1, and the emitted-byte prefix at the seam is neither 0 nor the byte count
        assert m.rs[seam] // rc.RT == rc.SC - 1 or L > rc.RT
        assert m.re[seam - 1] // rc.RT >= rc.SC
        assert 0 < m.G[seam] != seam
        f = rc.block_facts(m, rc.want(oracle, "c_seam_%d" % L, data, rc.C_SEAM_CAP), rc.C_SEAM_CAP)
        rc.check_model(f)
        assert len(f["S"]) > 40


def test_family_d_fast_path(oracle):
    tags = set()
    for name, cap in rc.family_d():
        assert 11000 <= cap <= 40000
        data = rc.inputs()[name]
        m, f = _facts(oracle, name, data, cap)
        tags |= rc.fast_path_tags(m, f)
    assert not rc.FAMILY_D_NEEDS - tags, "family D misses %s" % sorted(rc.FAMILY_D_NEEDS - tags)


def test_family_e_windows(oracle):
    for name, cap in rc.family_e():
        nb = len(rc.want(oracle, name, rc.inputs()[name], cap))
        assert nb >= 4 and any(nb % r for r in rc.E_RANGES)       # several windows, a partial last one
        assert nb <= 3000                                                         # (one rle1_finish per window: keep it quick)


def test_family_f_shares(oracle):
    seen = set()
    for name, (data, caps) in rc.family_f().items():
        tn = (data.size + rc.RT - 1) // rc.RT
        assert 40 <= tn <= 70
        m = rc.model(name, data)
        for world in rc.F_WORLDS:
            tpr = rc.tiles_per_rank(data.size, world)
            assert tpr % 4 == 0
            pw = rc.probe_windows(m, world)
            if None in pw:
                seen.add("rank_without_tiles")
            live = [p for p in pw if p]
            if any(p[0] >= 2 for p in live) and any(p[1] >= 2 for p in live):
                seen.add("probe_two_windows_each_way")
            if any(p[2] for p in live):
                seen.add("share_inside_one_run")
            borders = [r * tpr * rc.RT for r in range(1, world) if r * tpr < tn]
            for cap in caps:
                _, f = _facts(oracle, name, data, cap)
                if set(f["E"].tolist()) & set(borders):
                    seen.add("block_ends_with_last_byte_of_share")
                if set((f["E"] - 1).tolist()) & set(borders):
                    seen.add("block_ends_with_first_byte_of_share")
    # the run crosses a border with more than 16 KiB on each side
    m = rc.model("f_run", rc.family_f()["f_run"][0])
    b = rc.tiles_per_rank(m.n, 2) * rc.RT
    assert b - m.rs[b] > rc.WIN and m.re[b] - b > rc.WIN
    assert seen == {"rank_without_tiles", "probe_two_windows_each_way", "share_inside_one_run", "block_ends_with_last_byte_of_share",
                    "block_ends_with_first_byte_of_share"}, seen


def test_family_g_batch(oracle):
    cap, items = rc.family_g()
    d = dict(items)
    buf, se = rc.pack(items)
    assert sum(1 for s, _ in se if s & 1) >= 5 and {d[n].size for n in d} >= {1, 15, 16, 17, 4095, 4096, 4097, 8193}
    # the neighbours: one run of eight in the buffer, two runs for the kernels
    i = [n for n, _ in items].index("starts_zzzzz")
    s = se[i][0]
    mb = rc.Model(buf)
    assert se[i - 1][1] == s and mb.rs[s] == s - 3 and mb.re[s] == s + 5
    for x in (-1, 0, 1):
        for kind, flag in (("emits", False), ("absorbed", True)):
            data = d["E_cap%+d_%s" % (x, kind)]
            assert oracle.rle1_len(data) == cap + x and rc.absorbed_flag(data) == flag
            assert len(oracle.rle1_blocks_cap(data, cap)) == (1 if x < 0 or (x == 0 and not flag) else 2)
    for name, at in (("block_ends_at_4095", 4095), ("block_ends_at_4096", 4096)):
        assert oracle.rle1_blocks_cap(d[name], cap)[0][3] == at + 1           # with the tile's last byte / the next tile's first
        assert rc.Model(d[name]).re[0] > 255                                   # a chunk ends at offset 254 and the run goes on
    assert any(0 < b[3] % rc.RT < rc.RT - 1 for b in oracle.rle1_blocks_cap(d["five_blocks"], cap))      # and inside a tile
    blk = oracle.rle1_blocks_cap(d["cut_before_count"], cap)
    assert blk[0][0].size == cap and rc.Model(d["cut_before_count"][: blk[0][3]]).G[-1] == cap + 1      # the count lies at len
    assert len(oracle.rle1_blocks_cap(d["five_blocks"], cap)) == 5
    # the absorbed flag on both sides of its step, in inputs of one block (the flag is only read there)
    for T in rc.G_TAILS:
        data = d["tail_run_%d" % T]
        assert oracle.rle1_len(data) < cap and rc.Model(data).dp[-1] == (T - 1) % 255 and rc.absorbed_flag(data) == ((T - 1) % 255 >= 4)
    assert {(T - 1) % 255 for T in rc.G_TAILS} >= {2, 3, 4, 5, 254, 0}
    # rle_batch_len leaves its loop early: the first tile alone passes cap, more tiles follow
    assert rc.Model(d["len_8193"][: rc.RT]).G[-1] > cap and d["len_8193"].size > 2 * rc.RT


def test_family_h_sweep():
    h = rc.family_h()
    assert len(h) == rc.H_PAIRS == 200 and all(1 <= d.size <= 8192 for _, d, _ in h)
    assert {c for _, _, c in h} == set(rc.H_CAPS) and set(rc.H_CAPS) <= set(rc.CAPS_SMALL + rc.CAPS_255 + rc.CAPS_1275 + rc.CAPS_4096 + rc.CAPS_MOD5_1)
    lens = set()
    for _, d, _ in h:
        m = rc.Model(d)
        lens |= set((m.re - m.rs)[m.head].tolist())
    assert lens >= set(rc.RUNLENS)
    again = rc.family_h.__wrapped__()
    assert all(np.array_equal(a[1], b[1]) and a[2] == b[2] for a, b in zip(h, again))       # the seed fixes it
