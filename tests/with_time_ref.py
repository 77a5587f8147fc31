"""FIRSTWITHTIME / LASTWITHTIME restated in plain Python, independent of the engine's word packing.

Within a segment the docs of a group are offered in docId order and a doc takes over when its time is >= the best so
far (LAST, LastWithTimeAggregationFunction.java:112,147,196) or <= it (FIRST, FirstWithTimeAggregationFunction.java:
111,147,200). The segments' winners are then merged in bind order with the same comparison, the later segment as the
candidate: among equal winning times the greatest (segment bind index, docId) wins — the tie rule this library defines
where the reference leaves the merge order to its threads (:223 / :227).

numGroupsLimit (walk form): a segment admits the first `limit` distinct keys its matching docs show in docId order
(DictionaryBasedGroupKeyGenerator's first-seen cap); docs of other keys are dropped in that segment.
"""


def takes_over(function, time, best):
    return time >= best if function == "LASTWITHTIME" else time <= best


def segment_winners(function, times, keys, mask, limit=None):
    """{key: (doc, time)} of one segment: times / keys / mask are per-doc sequences (keys None: one group, key ())."""
    best, admitted = {}, set()
    for doc in range(len(times)):
        if not mask[doc]:
            continue
        k = () if keys is None else keys[doc]
        if limit is not None and k not in admitted:
            if len(admitted) >= limit:
                continue
            admitted.add(k)
        t = int(times[doc])
        if k not in best or takes_over(function, t, best[k][1]):
            best[k] = (doc, t)
    return best


def table_winners(function, segments, limit=None):
    """{key: (segment, doc, time)} over `segments` = [(times, keys, mask)] in bind order."""
    out = {}
    for si, (times, keys, mask) in enumerate(segments):
        for k, (doc, t) in segment_winners(function, times, keys, mask, limit).items():
            if k not in out or takes_over(function, t, out[k][2]):
                out[k] = (si, doc, t)
    return out


def brute_force(function, segments):
    """The same winners by sorting every matching (time, segment, doc) of a group: the extreme time, then the greatest
    (segment, doc)."""
    rows = {}
    for si, (times, keys, mask) in enumerate(segments):
        for doc in range(len(times)):
            if mask[doc]:
                rows.setdefault(() if keys is None else keys[doc], []).append((int(times[doc]), si, doc))
    out = {}
    for k, r in rows.items():
        t = max(x[0] for x in r) if function == "LASTWITHTIME" else min(x[0] for x in r)
        _, si, doc = max(x for x in r if x[0] == t)
        out[k] = (si, doc, t)
    return out
