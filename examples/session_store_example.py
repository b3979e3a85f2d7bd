"""Users who come back: keep the histories on the GPU and serve requests that only name users (Recommender.open_sessions).  A click
stream arrives as (user, item) events; every event appends one item to one user's history on the device, and a request for
recommendations sends user keys, not histories.  The lists are recommend_batch's lists for the same histories.

Runs on a synthetic log with a freshly initialised encoder; give the directory of a saved model (bert4rec_ml_1m_example.py or
bert4rec_lifecycle_example.py write one) to serve a trained one."""
import argparse
import pathlib

from _common import config, dataloaders, datasets, models, networks

from bert4rec_amd.apps import Recommender
from bert4rec_amd.models import model_utils

if __name__ == "__main__":
    parser = argparse.ArgumentParser(description=__doc__)
    parser.add_argument("model", nargs="?", default=None, help="a saved model; default: an untrained ml-1m_64 encoder")
    parser.add_argument("--users", type=int, default=200)
    parser.add_argument("--k", type=int, default=5)
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
    sessions = app.open_sessions(max_users=10_000)

    # the log so far, in arrival order: user u clicked through a window of the catalogue
    log = dataloader.create_item_list()
    events = [("user-%03d" % (n % args.users), log[n]) for n in range(40 * args.users)]
    accepted = sessions.append([u for u, _ in events], [i for _, i in events])
    print("%d events, %d accepted, %d users in the store (%d items kept per user)" % (len(events), accepted, len(sessions), sessions.history_capacity))

    # a request names users; "nobody yet" has no history and is served as a cold user
    asked = ["user-000", "user-001", "nobody yet"]
    for user, items in zip(asked, sessions.recommend(asked, k=args.k)):
        print("%-10s -> %s" % (user, items))

    # the same lists as from the full histories
    histories = [[i for u, i in events if u == user] for user in asked]
    assert sessions.recommend(asked, k=args.k) == app.recommend_batch(histories, k=args.k)
    assert sessions.history("user-000") == histories[0][-sessions.history_capacity:]

    # user-000 clicks on the first recommendation: one event, and the next request already knows it
    clicked = sessions.recommend(["user-000"], k=1)[0]
    sessions.append(["user-000"], [clicked])
    print("user-000 clicked %r -> %s" % (clicked, sessions.recommend(["user-000"], k=args.k)[0]))

    # a store survives a restart: CPU tensors and the key list
    saved = sessions.state_dict()
    restored = app.open_sessions(max_users=10_000)
    restored.load_state_dict(saved)
    assert restored.recommend(asked, k=args.k) == sessions.recommend(asked, k=args.k)
    sessions.forget(["user-001"])
    print("after forget: %d users; user-001 is cold again -> %s" % (len(sessions), sessions.recommend(["user-001"], k=args.k)[0]))
