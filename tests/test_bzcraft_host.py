"""No GPU: the crafted-header cases (bzcraft_cases.py) are what they claim, and the model decoder of bzcraft.py and the oracle's
decoder agree on every one of them -- same accept or reject, same bytes.  test_gpu_crafted_headers.py holds the HIP decoder to
the oracle on the same streams; what a case proves about a seam of the parallel header code is asserted here, from the bit
offsets the writer returns."""
import pytest

import bzcraft
import bzcraft_cases as cc


@pytest.mark.parametrize("name", [c.name for c in cc.CASES])
def test_model_and_oracle_agree_and_the_case_is_what_it_claims(oracle, name):
    case = cc.BY_NAME[name]
    data = case.stream()
    got = bzcraft.model(data)
    rc, out = oracle.bzip2_decompress(data)
    if case.expect == "ok":
        assert not isinstance(got, str), got
        assert rc == 0
        assert out.size == len(got) and out.tobytes() == got, name
        assert len(got) > 0
    else:
        assert got == case.expect                    # the reference line that rejects it
        assert rc == bzcraft.status_of(got) == (bzcraft.OBSOLETE_INPUT if name == "U-randomised-bit" else bzcraft.DATA_ERROR)
    if case.claim is not None:
        case.claim(case.blocks())


def test_every_family_is_there():
    count = {f: sum(1 for c in cc.CASES if c.family == f) for f in cc.FAMILIES}
    assert all(count.values()), count
    assert sum(count.values()) == len(cc.CASES)
    assert {c.expect for c in cc.CASES} >= {"ok", "selectors-run-out:1601", "randomised:1446", "group-count:1471", "n-sel:1478", "selector:1490",
                                            "length:1509", "no-code:1608", "run-size:1647", "size:1663"}


def test_the_writer_refuses_a_symbol_without_a_code():
    over = bzcraft.Table([2, 2, 1, 2, 1])            # both 1-bit values are codes: no 2-bit code is ever read
    assert over.code(2) == "0" and over.code(4) == "1"
    for sym in (0, 1, 3):
        with pytest.raises(bzcraft.NoCode):
            over.code(sym)
    three = bzcraft.Table([3, 2, 2, 2, 1])
    assert [three.code(s) for s in (4, 1, 2)] == ["0", "10", "11"]
    for sym in (0, 3):
        with pytest.raises(bzcraft.NoCode):
            three.code(sym)
    with pytest.raises(bzcraft.NoCode):
        cc.block(used=(65, 66, 67), tables=[cc.tab([2, 2, 1, 2, 1])] * 2, selectors=[0], symbols=[2, 3])
    assert [bzcraft.Table([2, 2, 3, 3, 3]).code(s) for s in range(5)] == ["00", "01", "100", "101", "110"]


def test_selector_values_follow_the_zero_initialised_list():
    assert bzcraft.unmtf_selectors([3, 1, 2, 0, 1], 3) == [0, 0, 1, 1, 0]      # the zero behind the three tables moves to the front
    assert bzcraft.unmtf_selectors([1, 2, 2, 1, 2, 0], 2) == [1, 0, 0, 0, 1, 1]


def test_all_ones_lane_words_in_the_alternating_tables():
    # 38 ones per drop from 20 to 1: over the 32 shifts some drop covers a whole 32-bit lane word (the decoder's m_ao), in every
    # stretch position class; two such words next to each other need 64 ones, which only the walk-to-0 cases have
    ao = {}
    for k in range(32):
        b = cc.BY_NAME["L-alternating-shift-%d" % k].blocks()[0]
        words = b.lane_words(b.tab[2][1], b.tab[2][2])
        ao[k] = [i for i, w in enumerate(words) if w == "1" * 32]
        assert not any(x + 1 == y for x, y in zip(ao[k], ao[k][1:]))
    assert sum(1 for k in ao if ao[k]) >= 1
    assert all(ao[k] for k in ao), "every shift has an all-ones lane word"
    assert any(i % 64 == 0 for k in ao for i in ao[k]) and any(i % 64 == 63 for k in ao for i in ao[k]), "in lane 0 and in lane 63"
    pairs = 0
    for k in (0, 5, 13, 26, 31):
        b = cc.BY_NAME["L-walk-to-0-ones-%d" % k].blocks()[0]
        words = b.lane_words(b.tab[1][1], b.tab[1][2])
        pairs += sum(1 for x, y in zip(words, words[1:]) if x == y == "1" * 32)
    assert pairs >= 5


def test_second_blocks_start_at_every_bit_of_a_word():
    starts = {(32 + cc.BY_NAME["S-second-block-at-bit-%d" % k].blocks()[0].bits.size) % 32 for k in range(32)}
    assert starts == set(range(32))


def test_run_digits():
    for n in (1, 2, 3, 16, 17, 5000, 99998):
        total = sum((d + 1) << i for i, d in enumerate(cc.run_digits(n)))
        assert total == n
