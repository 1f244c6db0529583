"""
The reference's three image queues (mpunet/image/queue/{eager,lazy,limitation}_queue.py, loading_pool.py, utils.py) over a
list of FILE ENTRIES: what `mp train --max_loaded_images N --num_access K` and `mp predict --dataset` hold in HBM at a time.

  EagerQueue        every entry resident, as without a queue
  LazyQueue         iterates the entries with ONE read ahead: while volume i is in use, a thread reads the file of i + 1
  LimitationQueue   limitation_queue.py member by member: at most `max_loaded` entries loaded; a FIFO of (entry, n_accesses);
                    an entry released with n_accesses >= num_access is unloaded, goes to the back of the non-loaded queue,
                    and ONE new load is requested; otherwise it is re-queued with n_accesses + 1. The first max_loaded + 1
                    arrivals start at a random count in [0, int(0.75 * num_access)) so that they do not all expire together.

THE THREADING RULE. A loader thread does FILE WORK ONLY -- read, gunzip, header parse (data.read_volume_host), into pageable
host memory -- and makes NO call into HIP or torch's device API: pipeline.TrainPipeline re-captures the train step's graph
whenever the learning rate moves, and a device call from another thread during a capture invalidates it. What a loader leaves
is a host payload (VolumeEntry.payload). The thread that cuts batches ADOPTS it (VolumeEntry.adopt: the one host-to-device
copy, mpu_volume_decode, the scaler fit) on its own current stream, at a batch boundary (data.TrainSampler takes its volumes
before it cuts). A volume's tensors are used on the stream they were allocated on; another stream that reads them is marked
with record_stream (data.TrainSampler does). Unloading drops the entry's references; the sampler drops its cache entry for the
volume, and torch's caching allocator hands the memory on in stream order.

Differences from the reference, on purpose: the pool calls a dataset's put / error functions from the loader thread itself (the
reference has two gather threads for it); a failed entry goes back to the non-loaded queue instead of ALSO entering the loaded
one (loading_pool.py:20-27 puts a failed image on both); the load queue is unbounded (the reference sleeps when it fills); when
every entry of a set has failed in a row no further load is requested, so that the caller gets the reference's Empty error
instead of a spinning pool. The timeout of that error is a constructor argument (5 s there).
"""
import threading
from contextlib import contextmanager
from queue import Queue, Empty

import numpy as np


def _warn_fn(logger):
    if logger is None:
        return lambda msg: print("[WARNING] " + msg, flush=True)
    w = getattr(logger, "warn", None)
    return w if w is not None else (lambda msg: logger("[WARNING] " + msg))


class VolumeEntry:
    """One volume of a dataset: where it comes from, and -- while it is loaded -- its host payload (left by a loader thread) or
    its resident volume (made of the payload by the thread that uses it)."""

    def __init__(self, path=None, label_path=None, identifier=None, loader=None, adopter=None):
        if identifier is None:
            from .nifti import volume_identifier
            identifier = volume_identifier(path)
        self.path, self.label_path, self.identifier = path, label_path, identifier
        self._loader, self._adopter = loader, adopter
        self.payload, self.volume = None, None

    @property
    def is_loaded(self):
        return self.payload is not None or self.volume is not None

    def load_host(self):
        """LOADER THREAD: file work only."""
        self.payload = self._loader(self)

    def adopt(self):
        """USING THREAD, its current stream: payload -> resident volume (no adopter: the payload itself)."""
        if self.volume is None:
            if self.payload is None:
                raise RuntimeError("entry %s is not loaded" % self.identifier)
            self.volume = self._adopter(self, self.payload) if self._adopter is not None else self.payload
            self.payload = None
        return self.volume

    def unload(self):
        self.payload, self.volume = None, None

    def __repr__(self):
        return "VolumeEntry(%s%s)" % (self.identifier, ", loaded" if self.is_loaded else "")


class Dataset:
    """A named list of entries (the ImagePairLoader of the reference's queues)."""

    def __init__(self, entries, identifier="dataset"):
        self.entries, self.identifier = list(entries), identifier

    def __len__(self):
        return len(self.entries)

    def __bool__(self):
        return len(self.entries) > 0

    def __repr__(self):
        return "%s (%d volumes)" % (self.identifier, len(self.entries))


def as_dataset(entries, identifier="dataset"):
    return entries if isinstance(entries, Dataset) else Dataset(entries or [], identifier)


class LoadingPool:
    """n_threads daemon threads that run VolumeEntry.load_host and hand the entry to its dataset's put function, or on an
    exception warn and hand it to the dataset's error function (loading_pool.py)."""

    def __init__(self, n_threads=3, logger=None):
        self.warn = _warn_fn(logger)
        self.thread_lock = threading.Lock()
        self._jobs = Queue()
        self._registered = {}
        self.pool = [threading.Thread(target=self._work, daemon=True) for _ in range(int(n_threads))]
        for t in self.pool:
            t.start()

    def _work(self):
        while True:
            job = self._jobs.get()
            try:
                if job is None:
                    return
                entry, dataset_id = job
                put, on_error = self._registered[dataset_id]
                try:
                    entry.load_host()
                except Exception as e:                          # noqa: BLE001 (any load error: warn, replace)
                    with self.thread_lock:
                        self.warn("[ERROR in LoadingPool] Could not load image '{}': {}".format(entry, e))
                    on_error(entry)
                else:
                    put(entry)
            finally:
                self._jobs.task_done()

    def qsize(self):
        return self._jobs.qsize()

    def join(self):
        self._jobs.join()

    def close(self):
        """End the threads (after the jobs already queued)."""
        for _ in self.pool:
            self._jobs.put(None)
        for t in self.pool:
            t.join()
        self.pool = []

    def add_image_to_load_queue(self, entry, dataset_id):
        if dataset_id not in self._registered:
            raise RuntimeError("Dataset {} is not registered. Call LoadingPool.register_dataset before adding items from "
                               "that dataset to the loading queue".format(dataset_id))
        self._jobs.put((entry, dataset_id))

    def register_dataset(self, dataset_id, load_put_function, error_put_function):
        with self.thread_lock:
            if dataset_id in self._registered:
                raise RuntimeWarning("A dataset of ID {} has already been registered.".format(dataset_id))
            self._registered[dataset_id] = (load_put_function, error_put_function)

    def de_register_dataset(self, dataset_id):
        with self.thread_lock:
            del self._registered[dataset_id]


class BaseQueue:
    def __init__(self, dataset, logger=None):
        self.dataset = as_dataset(dataset)
        self.logger = logger or (lambda *a, **k: None)
        self.warn = _warn_fn(logger)

    def __len__(self):
        return len(self.dataset)

    @property
    def entries(self):
        return self.dataset.entries

    @property
    def n_resident(self):
        """Entries that hold a host payload or a resident volume right now."""
        return sum(1 for e in self.dataset.entries if e.is_loaded)


class EagerQueue(BaseQueue):
    """Everything resident, loaded by the calling thread when the queue is built; `volumes` is the list a sampler indexes."""

    def __init__(self, dataset, logger=None, seed=None, **kwargs):
        super().__init__(dataset, logger)
        self.logger("'Eager' queue created:\n  Dataset:      {}".format(self.dataset))
        self.logger("Preloading all {} images now... (eager)".format(len(self.dataset)))
        self.volumes = []
        for e in self.entries:
            if not e.is_loaded:
                e.load_host()
            self.volumes.append(e.adopt())
        self._rng = np.random.RandomState(seed)

    @contextmanager
    def get_random_image(self):
        yield self.volumes[self._rng.randint(0, len(self.volumes))]


class LazyQueue(BaseQueue):
    """Volumes just in time. Iterating yields every entry's volume in list order; the file of the NEXT entry is read by one
    thread meanwhile (file work only), and an entry is unloaded when the loop moves on: at most the current and the next one
    are loaded. An entry that follows itself in the list is loaded once and kept for both turns."""

    def __init__(self, dataset, logger=None, seed=None, **kwargs):
        super().__init__(dataset, logger)
        self.logger("'Lazy' queue created:\n  Dataset:      {}".format(self.dataset))
        self.logger("Images will be loaded just-in-time and unloaded when not in use.")
        self._rng = np.random.RandomState(seed)

    @contextmanager
    def get_image_by_idx(self, idx):
        e = self.entries[idx]
        if not e.is_loaded:
            e.load_host()
        try:
            yield e.adopt()
        finally:
            e.unload()

    @contextmanager
    def get_random_image(self):
        with self.get_image_by_idx(self._rng.randint(0, len(self.entries))) as v:
            yield v

    def __iter__(self):
        entries = self.entries
        if not entries:
            return
        box = {}

        def read(e):
            try:
                e.load_host()
            except BaseException as err:                        # noqa: BLE001 (re-raised on the iterating thread)
                box[id(e)] = err

        def start(e):
            t = threading.Thread(target=read, args=(e,), daemon=True)
            t.start()
            return t

        ahead, nxt = start(entries[0]), entries[0]
        held = None                                             # the entry whose volume the loop holds right now
        try:
            for i, e in enumerate(entries):
                if ahead is not None:
                    ahead.join()
                ahead, nxt = None, None
                if id(e) in box:
                    raise box.pop(id(e))
                vol = e.adopt()                                 # (before the next read starts: its payload is dropped here)
                held = e
                # a list may name one entry twice in a row (mp train_fusion draws with replacement and repeats images to fill a
                # round): the volume then stays for the next turn -- a read ahead would put a payload into the entry that the
                # unload below drops again
                again = i + 1 < len(entries) and entries[i + 1] is e
                if i + 1 < len(entries) and not again:
                    ahead, nxt = start(entries[i + 1]), entries[i + 1]
                try:
                    yield vol
                finally:
                    del vol
                    if not again:
                        e.unload()
                        held = None
        finally:                                                # (a loop left early: nothing stays loaded, no thread is left)
            if ahead is not None:
                ahead.join()
                nxt.unload()
            if held is not None:
                held.unload()


class LimitationQueue(BaseQueue):
    """limitation_queue.py. `seed` shuffles the initial order (the first max_loaded entries of it are the preload: a seed all
    ranks share gives every replica the same first volumes); `rank_seed` shuffles the order in which the REST is loaded as
    replacements and draws the initial access offsets."""

    def __init__(self, dataset, max_loaded=25, num_access_before_reload=50, preload_now=True, await_preload=True,
                 loading_pool=None, n_load_jobs=3, logger=None, seed=None, rank_seed=None, timeout=5.0, **kwargs):
        super().__init__(dataset, logger)
        n = len(self.dataset)
        if n == 0:
            raise ValueError("LimitationQueue: dataset %s is empty" % self.dataset)
        self.max_loaded = min(max_loaded or n, n)
        self.num_access_before_reload = num_access_before_reload or 50
        self.timeout = float(timeout)
        self.loaded_queue = Queue(maxsize=self.max_loaded)
        self.non_loaded_queue = Queue(maxsize=n)
        self._lock = threading.Lock()
        self._rng = np.random.RandomState(rank_seed)
        inds = np.arange(n)
        np.random.RandomState(seed).shuffle(inds)
        tail = inds[self.max_loaded:].copy()
        self._rng.shuffle(tail)
        self.initial_order = [self.entries[i].identifier for i in inds[:self.max_loaded]]
        self.replacement_order = [self.entries[i].identifier for i in tail]
        for i in list(inds[:self.max_loaded]) + list(tail):
            self.non_loaded_queue.put(self.entries[i])
        self._own_pool = loading_pool is None
        self.loading_pool = loading_pool or LoadingPool(n_threads=n_load_jobs, logger=logger)
        self.loading_pool.register_dataset(dataset_id=self.dataset.identifier,
                                           load_put_function=self._add_loaded_to_queue,
                                           error_put_function=self._load_error_callback)
        self.max_offset = int(self.num_access_before_reload * 0.75)
        self.n_offset = self.max_loaded
        self._errors_in_a_row = 0
        self.n_loading = 0                                      # loads requested and not yet arrived (or failed)
        self.logger("'Limitation' queue created:\n  Dataset:      {}\n  Max loaded:   {}\n  Reload limit: {}".format(
            self.dataset, self.max_loaded, self.num_access_before_reload))
        if preload_now:
            self.preload(await_preload)

    def preload(self, await_preload=True):
        self.logger("Adding {} ImagePair objects from {} to load queue".format(self.max_loaded, self.dataset.identifier))
        if self.n_resident != 0 or self.loaded_queue.qsize() != 0:
            raise RuntimeError("Dataset {} seems to have already been loaded. Do not load any data before passing the "
                               "entries to the queue class. Only call LimitationQueue.preload once."
                               "".format(self.dataset.identifier))
        self._add_images_to_load_queue(num=self.max_loaded)
        if await_preload:
            self.logger("... awaiting preload")
            self.loading_pool.join()
            self.logger("Preload complete.")

    def close(self):
        if self._own_pool:
            self.loading_pool.close()

    def _warn_access_limit(self, min_fraction=0.10):
        qsize = self.loaded_queue.qsize()
        if qsize == 0:
            self.warn("Study ID queue for dataset {} seems to block. This might indicate a data loading "
                      "bottleneck.".format(self.dataset.identifier))
        elif qsize <= self.max_loaded * min_fraction:
            self.warn("Dataset {}: Loaded queue in too empty (qsize={}, maxsize={})".format(
                self.dataset.identifier, qsize, self.max_loaded))

    # ---- the two halves of get_random_image, for a caller that cannot hold a `with` block open (data.TrainSampler) ------------
    def get(self):
        """(entry, n_accesses) from the front of the FIFO."""
        with self.loading_pool.thread_lock:
            self._warn_access_limit()
        try:
            return self.loaded_queue.get(timeout=self.timeout)
        except Empty as e:
            raise Empty("Could not get ImagePair from dataset {} with timeout of {} seconds. Consider increasing the "
                        "number of load threads / max loaded per dataset / access threshold".format(
                            self.dataset.identifier, self.timeout if self.timeout != int(self.timeout)
                            else int(self.timeout))) from e

    def release(self, entry, n_accesses, defer_unload=False):
        """_release_image. Returns True when the entry has reached its limit; with defer_unload the caller then still uses the
        volume and calls retire(entry) when it is done (the unload, the return to the non-loaded queue, the new load)."""
        if n_accesses >= self.num_access_before_reload:
            if not defer_unload:
                self.retire(entry)
            return True
        self.loaded_queue.put((entry, n_accesses + 1))
        return False

    def retire(self, entry):
        entry.unload()
        self.non_loaded_queue.put(entry)
        self._add_images_to_load_queue(num=1)

    @contextmanager
    def get_random_image(self):
        entry, n_accesses = self.get()
        try:
            yield entry.adopt()
        finally:
            self._release_image(entry, n_accesses)

    def _release_image(self, entry, n_accesses):
        self.release(entry, n_accesses)

    @contextmanager
    def get_image_by_id(self, image_id):
        raise NotImplementedError

    @contextmanager
    def get_image_by_idx(self, image_idx):
        raise NotImplementedError

    def _add_images_to_load_queue(self, num=1):
        for _ in range(num):
            entry = self.non_loaded_queue.get_nowait()          # Should never block!
            if entry.is_loaded:
                raise RuntimeWarning("Image {} in dataset {} seems to be already loaded, but it was fetched from the "
                                     "non_loaded_queue queue. This could be an implementation error!".format(
                                         entry.identifier, self.dataset.identifier))
            with self._lock:
                self.n_loading += 1
            self.loading_pool.add_image_to_load_queue(entry, self.dataset.identifier)

    def _add_loaded_to_queue(self, entry):
        with self._lock:
            self._errors_in_a_row = 0
            self.n_loading -= 1
            if self.n_offset >= 0:
                offset = int(self._rng.randint(0, self.max_offset)) if self.max_offset > 0 else 0
                self.n_offset -= 1
            else:
                offset = 0
        self.loaded_queue.put((entry, offset))

    def _load_error_callback(self, entry, *args, **kwargs):
        self.warn("Load error on image {}".format(entry))
        entry.unload()
        with self._lock:
            self.n_loading -= 1
            self._errors_in_a_row += 1
            again = self._errors_in_a_row < len(self.dataset)
        self.non_loaded_queue.put(entry)
        if again:
            self._add_images_to_load_queue(num=1)


QUEUE_TYPES = {"eager": EagerQueue, "lazy": LazyQueue, "limitation": LimitationQueue}


def validate_queue_type(queue_type, dataset, max_loaded, logger=None):
    if queue_type is LimitationQueue and (max_loaded is None or len(dataset) <= max_loaded):
        _warn_fn(logger)("Falling back to 'Eager' queue for dataset {} due to 'max_loaded' value of {} which is either 'None' "
                         "or larger than or equal to the total number of images ({}) in the dataset.".format(
                             dataset, max_loaded, len(dataset)))
        return EagerQueue
    return queue_type


def get_data_queues(train_dataset, val_dataset, train_queue_type, val_queue_type, max_loaded, num_access_before_reload,
                    logger=None, seed=None, rank_seed=None, timeout=5.0):
    """queue/utils.py: (train queue, validation queue or None). Both sets get the same rule; limitation queues share one
    loading pool of 3 threads. The training queue's preload is awaited, the validation queue's is not."""
    train_dataset = as_dataset(train_dataset, "train_data")
    val_dataset = as_dataset(val_dataset, "val_data") if val_dataset else None
    train_queue = validate_queue_type(QUEUE_TYPES[train_queue_type.lower()], train_dataset, max_loaded, logger)
    if val_queue_type and val_dataset:
        val_queue = validate_queue_type(QUEUE_TYPES[val_queue_type.lower()], val_dataset, max_loaded, logger)
    else:
        val_queue = None
    loading_pool = None
    if train_queue is LimitationQueue or val_queue is LimitationQueue:
        loading_pool = LoadingPool(n_threads=3, logger=logger)
    kw = dict(max_loaded=max_loaded, num_access_before_reload=num_access_before_reload, preload_now=True,
              loading_pool=loading_pool, logger=logger, timeout=timeout)
    train_queue = train_queue(dataset=train_dataset, await_preload=True, seed=seed, rank_seed=rank_seed, **kw)
    if val_queue is not None:
        val_queue = val_queue(dataset=val_dataset, await_preload=False, seed=None if seed is None else seed + 1,
                              rank_seed=None if rank_seed is None else rank_seed + 1, **kw)
    return train_queue, val_queue
