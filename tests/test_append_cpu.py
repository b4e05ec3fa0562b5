"""The host side of continuing on a kept KV cache (vz_hip/append.py) and the workspace arithmetic of the append attention: no GPU."""
import pytest
import torch

from vz_hip import append as AP

IMG = -200


def test_plan_accepts_a_proper_extension():
    p = AP.plan([[1, IMG, 5, 6, 7, 8, 9]], lengths=[40], ids=[[1, IMG, 5, 6]], next_pos=[40], image_token=IMG)
    assert p.suffix == [[7, 8, 9]] and p.past == [40] and p.next_pos == [40] and p.new_lens == [3] and p.width == 3
    assert p.history == [[1, IMG, 5, 6, 7, 8, 9]]          # what the filters' histories of the continued call start from


def test_plan_reports_the_first_differing_id():
    with pytest.raises(ValueError, match="index 2"):
        AP.plan([[1, 2, 9, 4, 5]], [4], [[1, 2, 3, 4]], None, IMG)
    with pytest.raises(ValueError, match="index 3"):          # the caller's ids end inside the cached part
        AP.plan([[1, 2, 3]], [4], [[1, 2, 3, 4]], None, IMG)


def test_plan_refuses_an_empty_suffix_and_an_image_in_it():
    with pytest.raises(NotImplementedError, match="no new id"):
        AP.plan([[1, 2, 3, 4]], [4], [[1, 2, 3, 4]], None, IMG)
    with pytest.raises(NotImplementedError, match="image"):
        AP.plan([[1, 2, 3, 4, 5, IMG, 6]], [4], [[1, 2, 3, 4]], None, IMG)
    AP.plan([[1, IMG, 3, 4, 5]], [40], [[1, IMG, 3, 4]], None, IMG)          # an image in the cached part is what a first turn leaves


def test_plan_row_count_and_idless_handles():
    with pytest.raises(ValueError, match="2 rows"):
        AP.plan([[1, 2], [3, 4]], [1], [[1]], None, IMG)
    # a handle of forward() holds positions, no ids: the suffix is what lies behind them, and the ids must reach that far
    p = AP.plan([[1, 2, 3, 4, 5, 6]], [4], None, None, IMG)
    assert p.suffix == [[5, 6]] and p.next_pos == [4]
    with pytest.raises(ValueError, match="holds 4"):
        AP.plan([[1, 2, 3]], [4], None, None, IMG)


def test_plan_per_row_lengths_left_and_right_padded():
    known = [[1, 2, 3], [4, 5, 6, 7, 8]]
    conv = [[1, 2, 3, 10, 11, 12, 13], [4, 5, 6, 7, 8, 20, 21]]
    for side in ("right", "left"):
        L = 9
        ids = torch.zeros(2, L, dtype=torch.long)
        mask = torch.zeros(2, L, dtype=torch.long)
        for b, r in enumerate(conv):
            sl = slice(0, len(r)) if side == "right" else slice(L - len(r), L)
            ids[b, sl] = torch.tensor(r)
            mask[b, sl] = 1
        rows = AP.masked_rows(ids, mask)
        assert rows == conv
        p = AP.plan(rows, lengths=[35, 5], ids=known, next_pos=[35, 5], image_token=IMG)
        assert p.suffix == [[10, 11, 12, 13], [20, 21]] and p.past == [35, 5] and p.new_lens == [4, 2] and p.width == 4
    assert AP.masked_rows([[1, 2], [3, 4]]) == [[1, 2], [3, 4]]
    with pytest.raises(ValueError):
        AP.masked_rows(torch.zeros(2, 3, dtype=torch.long), torch.ones(2, 4, dtype=torch.long))


def test_bookkeeping_all_emitted_ids_but_the_last():
    # row 0 ran its 4 tokens; row 1 stopped at its eos (2) after two and shows the fill id behind it
    seqs = [[11, 12, 13, 14], [21, 2, 0, 0]]
    counts = AP.emitted_counts(seqs, {2})
    assert counts == [4, 2]
    emitted = [r[:n] for r, n in zip(seqs, counts)]
    lengths, pos, ids = AP.after_generate([[1, IMG, 3], [4, 5]], prompt_positions=[34, 2], next_pos=[34, 2], emitted=emitted)
    assert lengths == [34 + 3, 2 + 1] and pos == [37, 3]
    assert ids == [[1, IMG, 3, 11, 12, 13], [4, 5, 21]]
    # one emitted id: nothing but the prompt is cached
    assert AP.after_generate([[1, 2]], [2], [2], [[9]]) == ([2], [2], [[1, 2]])
    # a row ended by a stop condition shows the fill id behind its stopping token; without fill the width counts
    assert AP.emitted_counts([[5, 6, 0, 0], [5, 6, 7, 8]], set(), fill=0) == [2, 4]
    assert AP.emitted_counts([[0, 0, 0]], set(), fill=0) == [1]
    assert AP.emitted_counts([[5, 6, 0, 0]], set()) == [4]
    # the next turn's plan accepts exactly what the bookkeeping says
    nxt = AP.plan([ids[0] + [14, 50, 51]], [lengths[0]], [ids[0]], [pos[0]], IMG)
    assert nxt.suffix == [[14, 50, 51]] and nxt.past == [37]


def test_append_min_new():
    assert AP.APPEND_MIN_NEW == 4


def test_workspace_floats_positive_and_monotone():
    from vz_hip import binding as B
    B.load_library()
    f = B.attention_append_ws_floats
    Hq, Hkv = 32, 8
    prev = 0
    for T in (1, 2, 3, 4, 15, 16, 17, 31, 33, 64, 65, 128, 130, 256, 1000):
        v = f(1, T, Hq, Hkv, 2048)
        assert v > 0 and v >= prev, (T, v, prev)
        prev = v
    for T in (1, 17, 130):
        prev = 0
        for ctx in (1, 63, 64, 65, 128, 512, 2048, 4096, 32768):
            v = f(2, T, Hq, Hkv, ctx)
            assert v > 0 and v >= prev, (T, ctx, v, prev)
            prev = v
    assert f(1, 0, Hq, Hkv, 512) == 0 and f(1, 4, 32, 5, 512) == 0          # shapes the op refuses
    assert B.stage_ws_bytes is not None and B.STAGE_APPEND == 4
