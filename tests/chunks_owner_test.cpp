// chunks_owner_test.cpp — the chunk table's owner (aukit_amd/csrc/chunks.h) on the host alone: create, shape, deliver, and an owner that
// leaves its scope undelivered.  Built and run by tests/test_chunks_owner_host.py; prints one line and returns 0 when every assert held.
#undef NDEBUG
#include <cassert>
#include <cstdio>
#include "../aukit_amd/csrc/chunks.h"

using namespace aukit;

static void all_zero(const aukit_chunks &c, size_t width) {
    assert(c.lens.size() == (size_t)c.n * width && c.pos.size() == (size_t)c.n * width);
    for (uint32_t v : c.lens) assert(v == 0);
    for (double v : c.pos) assert(v == 0);
}

int main() {
    {   // no streams: empty vectors, and still a row width of 1
        ChunksOwner ck = chunks_create(0);
        assert(ck && ck->n == 0 && ck->max_chunks == 0 && ck->channels == 1);
        assert(ck->nchunks.empty() && ck->status.empty() && ck->length_seconds.empty());
        assert(chunks_shape(*ck) == 1);
        all_zero(*ck, 1);
    }
    {   // streams without a single chunk: max_chunks stays 0, the rows are one entry wide
        ChunksOwner ck = chunks_create(3);
        assert(ck->n == 3 && ck->nchunks.size() == 3 && ck->status.size() == 3 && ck->length_seconds.size() == 3);
        for (uint32_t s = 0; s < 3; s++) {
            assert(ck->nchunks[s] == 0 && ck->status[s] == 0 && ck->length_seconds[s] == 0);
            chunks_set_count(*ck, s, 0);
        }
        assert(ck->max_chunks == 0);
        assert(chunks_shape(*ck) == 1);
        all_zero(*ck, 1);
    }
    {   // ragged counts: the widest stream sets the row width, and shaping zeroes what was there before
        ChunksOwner ck = chunks_create(4);
        const uint32_t counts[4] = {2, 0, 5, 1};
        for (uint32_t s = 0; s < 4; s++) chunks_set_count(*ck, s, counts[s]);
        assert(ck->max_chunks == 5);
        for (uint32_t s = 0; s < 4; s++) assert(ck->nchunks[s] == counts[s]);
        ck->lens.assign(7, 9u);
        ck->pos.assign(7, 9.0);
        const uint32_t mc = chunks_shape(*ck);
        assert(mc == 5);
        all_zero(*ck, 5);
        ck->lens[(size_t)2 * mc + 4] = 48000;   // the last chunk of the widest stream is the last entry of its row
        assert(ck->lens[14] == 48000);
    }
    {   // no handle: the table is dropped, the owner is empty, and a second delivery does nothing
        ChunksOwner ck = chunks_create(2);
        chunks_shape(*ck);
        chunks_deliver(ck, nullptr);
        assert(!ck);
        chunks_deliver(ck, nullptr);
        assert(!ck);
    }
    aukit_chunks *h = nullptr;
    {   // an empty handle takes the table
        ChunksOwner ck = chunks_create(2);
        chunks_set_count(*ck, 1, 3);
        chunks_shape(*ck);
        aukit_chunks *raw = ck.get();
        chunks_deliver(ck, &h);
        assert(!ck && h == raw && h->n == 2 && h->max_chunks == 3);
        chunks_deliver(ck, &h);   // delivered once: the empty owner leaves the handle alone
        assert(h == raw && h->n == 2);
    }
    {   // a handle that holds an older table: the old one is freed (the sanitizer build reports it otherwise), the new one installed
        ChunksOwner ck = chunks_create(5);
        chunks_set_count(*ck, 0, 1);
        chunks_shape(*ck);
        aukit_chunks *raw = ck.get();
        chunks_deliver(ck, &h);
        assert(!ck && h == raw && h->n == 5 && h->max_chunks == 1 && h->lens.size() == 5);
    }
    {   // an owner that goes out of scope undelivered (a driver's error return): the caller's handle is untouched and still readable
        aukit_chunks *before = h;
        {
            ChunksOwner ck = chunks_create(7);
            chunks_set_count(*ck, 6, 2);
            chunks_shape(*ck);
            assert(ck.get() != h);
        }
        assert(h == before && h->n == 5 && h->max_chunks == 1 && h->nchunks[0] == 1 && h->lens.size() == 5);
    }
    delete h;   // what aukit_chunks_free does
    printf("chunks owner: ok\n");
    return 0;
}
