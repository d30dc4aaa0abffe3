#!/usr/bin/env python
"""Drop-in demonstration: the reference's run_batch (/root/reference/train.py:17-63; tspgnn/train.py) running on
the MI355X path, over synthetic Euclidean instances (no Concorde, no dataset on disk).

    python examples/train_synthetic.py -d 64 -timesteps 32 -batchsize 8 -epochs 2 --batches 8
    python examples/train_synthetic.py --instances /tmp/tsp/instances --checkpoints /tmp/tsp/ckpt   # .graph files + resume
    python examples/train_synthetic.py -generate 512     # the reference's stream (n 20-40), drawn, labelled, packed on the GPU
    python examples/train_synthetic.py -accumulate 4     # one optimiser step per 4 batches: a step on 4 x the batch

The flags keep train.py's names (train.py:107-119).  Every instance appears twice in a batch with target
cost (1-dev) and (1+dev) times its tour cost and labels 0/1, exactly like InstanceLoader.get_batches
(instance_loader.py:16-27,82-87).  The "tour" is the planted Hamiltonian cycle, not the optimum, so the
accuracy printed here says nothing about TSP -- the point is the call sequence and the loss going down.
With -generate SAMPLES the instances are create_dataset's (seeded with -seed) and the tours are the GPU search's labels:
DeviceDataset.generate(SAMPLES, 20, 40), no matrix on the host and no file; -write_dir PATH also writes them as .graph
files (DeviceDataset.write_directory, formatted on the GPU) for the reference's train.py / test.py to read.
With --instances DIR -device_dataset -reader device the .graph files are parsed and packed on the GPU from their raw bytes
(DeviceDataset.from_directory(reader='device')) instead of one host parse per file.
-route_head [-route_loss W] trains the second per-edge head as well (build_network(d, route_head=True, route_loss=W)): a
sigmoid cross entropy of E_route against "this edge lies on the instance's tour", added to the decision loss with weight W.
The marks come from DeviceDataset(routes=True) with -device_dataset / -generate, or from route_edge_marks_host for the
synthetic batches; a decision-only checkpoint under --checkpoints starts such a run (load_weights(missing_ok=True)).
"""
import argparse
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tsp-gnn_amd"))
from tspgnn import (DeviceDataset, InstanceLoader, Session, build_network, global_variables_initializer, load_weights,  # noqa: E402
                    random_instance, route_edge_marks_host, save_weights, write_graph)
from tspgnn.train import run_batch, run_batches_accumulated, summarize_epoch  # noqa: E402


if __name__ == '__main__':
    p = argparse.ArgumentParser()
    p.add_argument('-d', default=64, type=int)
    p.add_argument('-timesteps', default=32, type=int)
    p.add_argument('-dev', default=0.02, type=float)
    p.add_argument('-epochs', default=2, type=int)
    p.add_argument('-batchsize', default=8, type=int)
    p.add_argument('-seed', default=42, type=int)
    p.add_argument('--batches', default=8, type=int, help='batches per epoch')
    p.add_argument('--instances', default=None, help='directory of .graph files (written with synthetic instances if '
                                                     'missing); batches then come from InstanceLoader.get_batches like train.py:178')
    p.add_argument('--checkpoints', default=None, help='directory for TensorFlow-format checkpoints: resumes from the '
                                                       'newest epoch=N found there and saves after every epoch (train.py:205)')
    p.add_argument('-device_dataset', action='store_true',
                   help='upload the instances once (tspgnn.DeviceDataset) and assemble every batch on the GPU from instance '
                        'ids: epochs through DeviceDataset.get_batches instead of InstanceLoader / create_batch')
    p.add_argument('-reader', default='host', choices=('host', 'device'),
                   help='with --instances DIR -device_dataset: who reads the .graph files (DeviceDataset.from_directory('
                        'reader=)): the host parser per file, or the GPU reader over chunks of raw text')
    p.add_argument('-generate', default=0, type=int, metavar='SAMPLES',
                   help='train on DeviceDataset.generate(SAMPLES, 20, 40): the instances drawn from the reference\'s stream, '
                        'labelled and packed on the GPU, instead of a directory or synthetic instances')
    p.add_argument('-write_dir', default=None, metavar='PATH',
                   help='with -generate: also write the generated instances to PATH as .graph files, formatted on the GPU')
    p.add_argument('-accumulate', default=1, type=int, metavar='K',
                   help='gradient accumulation: every K consecutive batches of an epoch form ONE optimiser step on their '
                        'union (run_batches_accumulated; a short last group is a smaller step); 1: a step per batch')
    p.add_argument('-route_head', action='store_true',
                   help='also train E_route, the per-edge head supervised by the tours\' edges (needs the tours with the '
                        'batches: synthetic instances, -device_dataset or -generate)')
    p.add_argument('-route_loss', default=1.0, type=float, metavar='W', help='with -route_head: the weight of the route loss')
    a = p.parse_args()
    if a.route_head and a.instances is not None and not a.device_dataset:
        p.error('-route_head with --instances DIR needs -device_dataset: InstanceLoader batches do not carry their tours')
    if a.accumulate < 1:
        p.error('-accumulate K needs K >= 1')
    if a.reader == 'device' and (a.instances is None or not a.device_dataset or a.generate):
        p.error('-reader device needs --instances DIR -device_dataset (and no -generate)')
    if a.write_dir is not None and not a.generate:
        p.error('-write_dir needs -generate SAMPLES')
    rng = np.random.RandomState(a.seed)
    loader = None
    if a.instances is not None:
        if not os.path.isdir(a.instances):
            os.makedirs(a.instances)
            for i in range(a.batchsize * a.batches):
                Ma, Mw, route = random_instance(int(rng.randint(20, 41)), rng)
                write_graph(Ma, Mw, os.path.join(a.instances, '{}.graph'.format(i)), route=route)
        loader = InstanceLoader(a.instances)
    dataset = None
    if a.generate:
        random.seed(a.seed)
        np.random.seed(a.seed)
        dataset = DeviceDataset.generate(a.generate, 20, 40, routes=a.route_head)
        t = dataset.summary['times']
        print('generated {} instances in {:.2f} s ({}); certified at dev 0.02: {:.3f}'.format(
            a.generate, t['total'], ', '.join('{} {:.3f}'.format(k, v) for k, v in t.items() if k != 'total'),
            dataset.summary['certified_fraction']), flush=True)
        if a.write_dir is not None:
            w = dataset.write_directory(a.write_dir)
            print('wrote {} bytes of .graph files to {} ({})'.format(
                w['bytes'], a.write_dir, ', '.join('{} {:.3f}'.format(k, v) for k, v in w['times'].items())), flush=True)
    elif a.device_dataset:   # the same instances every epoch, shuffled per epoch like InstanceLoader.reset()
        dataset = (DeviceDataset.from_directory(a.instances, reader=a.reader, routes=a.route_head)
                   if a.instances is not None else
                   DeviceDataset([random_instance(int(rng.randint(20, 41)), rng) for _ in range(a.batchsize * a.batches)],
                                 routes=a.route_head))
    GNN = build_network(a.d, route_head=a.route_head, route_loss=a.route_loss)
    with Session() as sess:
        sess.run(global_variables_initializer(seed=a.seed))
        first = 0
        if a.checkpoints is not None and os.path.isdir(a.checkpoints):
            saved = sorted(int(x.split('=')[1]) for x in os.listdir(a.checkpoints) if x.startswith('epoch='))
            if saved:
                first = load_weights(sess, '{}/epoch={}'.format(a.checkpoints, saved[-1]), missing_ok=a.route_head) + 1
        for epoch in range(first, first + a.epochs):
            stats = []
            if dataset is not None:
                batches = dataset.get_batches(a.batchsize, a.dev, a.timesteps, rng=rng)
            elif loader is not None:
                loader.reset()
                batches = loader.get_batches(a.batchsize, a.dev)
            else:
                def synthetic():
                    for _ in range(a.batches):
                        base = [random_instance(int(rng.randint(20, 41)), rng) for _ in range(a.batchsize)]
                        twice = [inst for inst in base for _ in (0, 1)]
                        batch = InstanceLoader.create_batch(twice, dev=a.dev)
                        yield batch + (route_edge_marks_host(twice)[0],) if a.route_head else batch
                batches = synthetic()
            if a.accumulate == 1:
                for b, batch in enumerate(batches):
                    stats.append(run_batch(sess, GNN, batch, b, epoch, a.timesteps, train=True)[:4])
            else:
                group, step = [], 0
                for batch in batches:
                    group.append(batch)
                    if len(group) == a.accumulate:
                        stats.append(run_batches_accumulated(sess, GNN, group, step, epoch, a.timesteps)[:4])
                        group, step = [], step + 1
                if group:
                    stats.append(run_batches_accumulated(sess, GNN, group, step, epoch, a.timesteps)[:4])
            summarize_epoch(epoch, *zip(*stats), train=True)
            if a.checkpoints is not None:
                save_weights(sess, '{}/epoch={}'.format(a.checkpoints, epoch))
