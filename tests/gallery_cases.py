"""What the gallery tests share: the pinned maps of seed 1 (tests/test_gpu_found_attractors.py: FOUND) with the `extent` of their
search records — the raw bounding box of the 20000 phase-2 points at the search's defaults — written in as constants, so that a
view is framed from a record without running the search. (tests/search_restatement.py: search(1, candidate, 1) prints them; the
restatement's records are the device's, bit for bit.)"""
SEED = 1
_H = float.fromhex
EXTENT = {
    # lossy: a third of its render jobs leave for infinity; flat in z
    545: tuple(map(_H, ("-0x1.c98c418c3669bp-1", "0x1.13e7ad3f6d5ffp-2", "-0x1.18dd87d2fb305p-1", "0x1.dabbbf1b63138p-5",
                        "-0x1.9a6106a5e7db1p-3", "0x1.c024f30761c38p-3"))),
    # the widest: about 2 x 1.9 x 3
    2573: tuple(map(_H, ("-0x1.d7b5a63863db3p+0", "0x1.a6106ac0b6e1cp-3", "-0x1.71f3adfeea5bep+0", "0x1.ec322b092d0d9p-2",
                         "-0x1.767c7c96f4139p+0", "0x1.962ad1d2791e6p+0"))),
    # flat in y, barely chaotic
    6377: tuple(map(_H, ("-0x1.3aa41e2cfad05p-1", "0x1.64d53c31f481dp-2", "-0x1.1df7c6d9a5369p+0", "0x1.19fb31b3f56f8p-5",
                         "0x1.033df687a5decp-2", "0x1.d6854bbf9947ep-1"))),
    # the highest Kaplan-Yorke dimension found (2.62)
    3944: tuple(map(_H, ("-0x1.43ae20d0247cfp-1", "0x1.0ce5430686416p-1", "-0x1.11d88bc7c3523p-1", "0x1.49c0067a1a5c5p-1",
                         "0x1.774538a02ddfap-4", "0x1.12b7b7a1f1f40p+0"))),
}
