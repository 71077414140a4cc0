"""The two helpers every XCD-aware table layout shares (hypelcnn_amd/gemm_tables.py): the eight contiguous shares the
kernels' XCD remap hands out, and the heaviest-first deal onto the least loaded XCD.  Expected values by hand.  CPU only."""
from hypelcnn_amd.gemm_tables import xcd_deal, xcd_shares


def test_eight_contiguous_shares():
    assert xcd_shares([]) == [[], [], [], [], [], [], [], []]
    assert xcd_shares(list(range(7))) == [[0], [1], [2], [3], [4], [5], [6], []]
    assert xcd_shares(list(range(8))) == [[0], [1], [2], [3], [4], [5], [6], [7]]
    # 13 = 8 x 1 + 5: the first five shares are one longer
    assert xcd_shares(list(range(13))) == [[0, 1], [2, 3], [4, 5], [6, 7], [8, 9], [10], [11], [12]]


def test_deal_ties_go_to_the_lowest_index():
    items = [(name, 5) for name in "abcdefghi"]  # nine equal items on eight empty XCDs: the ninth is back at XCD 0
    dealt, loads = xcd_deal(items, lambda it: it[1])
    assert dealt == [[("a", 5), ("i", 5)], [("b", 5)], [("c", 5)], [("d", 5)], [("e", 5)], [("f", 5)], [("g", 5)], [("h", 5)]]
    assert loads == [10, 5, 5, 5, 5, 5, 5, 5]


def test_deal_is_heaviest_first_and_keeps_the_order_of_equals():
    dealt, loads = xcd_deal([("s", 1), ("l", 9), ("m1", 5), ("m2", 5)], lambda it: it[1])
    assert dealt == [[("l", 9)], [("m1", 5)], [("m2", 5)], [("s", 1)], [], [], [], []]
    assert loads == [9, 5, 5, 1, 0, 0, 0, 0]


def test_deal_onto_starting_loads():
    start = [0, 5, 5, 5, 5, 5, 5, 1]
    # 4 -> XCD 0 (0 -> 4); 3 -> XCD 7 (1 -> 4); 2 -> XCDs 0 and 7 tie at 4: XCD 0
    dealt, loads = xcd_deal([2, 3, 4], lambda w: w, start)
    assert dealt == [[4, 2], [], [], [], [], [], [], [3]]
    assert loads == [6, 5, 5, 5, 5, 5, 5, 4]
    assert start == [0, 5, 5, 5, 5, 5, 5, 1], "the caller's loads are not modified"
