"""Limited items: 200 users, a promotion with a few coupons per film (Recommender.allocate).  recommend_batch hands the most popular
item to everybody; with a stock, every item is given at most as often as there are units of it, a contended item goes to the users
most likely to take it, and whoever loses it gets the next item of their own list instead.  The second half serves two waves of users
from one stock (first come, first served across calls) and the same from a session store.

Runs on a synthetic log with a freshly initialised encoder; give the directory of a saved model (bert4rec_ml_1m_example.py or
bert4rec_lifecycle_example.py write one) to serve a trained one."""
import argparse
import collections
import pathlib

from _common import config, dataloaders, datasets, models, networks

from bert4rec_amd.apps import Recommender
from bert4rec_amd.models import model_utils

if __name__ == "__main__":
    parser = argparse.ArgumentParser(description=__doc__)
    parser.add_argument("model", nargs="?", default=None, help="a saved model; default: an untrained ml-1m_64 encoder")
    parser.add_argument("--users", type=int, default=200)
    parser.add_argument("--k", type=int, default=5)
    parser.add_argument("--units", type=int, default=3, help="coupons per limited item")
    args = parser.parse_args()
    kwargs, model = {}, None
    if args.model is not None:
        loaded = models.BERT4RecModelWrapper.load(model_utils.determine_model_path(pathlib.Path(args.model)))
        kwargs = {"tokenizer": loaded["tokenizer"]} if "tokenizer" in loaded else {}
        model = loaded["model_wrapper"].model
    if not datasets.ML1M.is_available():
        kwargs["data_source"] = datasets.synthetic_dataset(n_users=1500, n_items=3706, min_len=20, max_len=200, seed=0, order=0.6)
    dataloader = dataloaders.get_dataloader_factory("bert4rec").create_ml_1m_dataloader(**kwargs)
    dataloader.generate_vocab()
    if model is None:
        model = models.BERT4RecModel(networks.Bert4RecEncoder(dataloader.get_tokenizer().get_vocab_size(), **config.get_encoder_config("ml-1m_64")))
    app = Recommender(model, dataloader)

    log = dataloader.create_item_list()
    histories = [log[37 * u:37 * u + 20 + u % 30] for u in range(args.users)]

    # without a stock: how often is each item handed out?
    plain = app.recommend_batch(histories, k=args.k)
    handed = collections.Counter(item for row in plain for item in row)
    print("recommend_batch: the most recommended items -> %s" % handed.most_common(3))

    # the 20 most recommended items are on promotion, `units` coupons each; everything else is unlimited
    stock = {item: args.units for item, _ in handed.most_common(20)}
    lists, left = app.allocate(histories, stock, k=args.k)
    given = collections.Counter(item for row in lists for item, _ in row)
    assert all(given[item] + left[item] == units for item, units in stock.items()) and all(len(row) == args.k for row in lists)
    print("allocate: %d of %d coupons given, no item more than %d times; the same three items now -> %s"
          % (sum(stock.values()) - sum(left.values()), sum(stock.values()), args.units, [(item, given[item]) for item, _ in handed.most_common(3)]))
    changed = sum([item for item, _ in row] != list(p) for row, p in zip(lists, plain))
    print("%d of %d users got a list that differs from their plain top %d; user 0: %s" % (changed, args.users, args.k, lists[0]))

    # two waves from one stock: what the first wave leaves is the stock of the second (first come, first served)
    half = args.users // 2
    first, left_1 = app.allocate(histories[:half], stock, k=args.k)
    second, left_2 = app.allocate(histories[half:], left_1, k=args.k)
    print("two waves: %d coupons left after the first, %d after the second (one call for everybody leaves %d)"
          % (sum(left_1.values()), sum(left_2.values()), sum(left.values())))

    # the same from a session store: the request names users
    sessions = app.open_sessions(max_users=10_000)
    keys = ["user-%03d" % u for u in range(args.users)]
    sessions.append([k for k, h in zip(keys, histories) for _ in h], [i for h in histories for i in h], return_accepted=False)
    assert sessions.allocate(keys, stock, k=args.k) == (lists, left)
    print("the session store allocates the same lists")
