"""Train a Bayesian neural network, then ask it for predictions: the second half of the reference's classification scripts
(tests/test_MNIST_bayesian_neural_network.py:66-81).

    hidden = BF.tanh(BF.matmul(weights1, x) + b1);   k ~ CategoricalVariable(logits=BF.matmul(weights2, hidden) + b2)

Nothing is downloaded, so there is no MNIST: the features are synthetic integer counts and the labels what a fixed random linear map of
them ranks highest (`teacher=`), so that there is something to learn and a second draw of features is held-out data of the same task.
After training, `CompiledBnn.predict` draws N weight sets from the posterior, runs the network forward on the held-out rows on the
matrix cores and returns the predictive mean per class; the reference's own call, `model._get_posterior_sample(N, input_values={x:
rows})[k]`, answers from the same pass.  Run on a machine with an MI355X:

    python examples/bnn_predict.py [iterations] [learning rate]
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from brancher_amd import engine, inference, workloads as W

ITERATIONS = int(sys.argv[1]) if len(sys.argv) > 1 else 3000
LR = float(sys.argv[2]) if len(sys.argv) > 2 else 5e-3
# 64 integer features (-3 .. 3: exactly bf16, so training and prediction run on the bf16 matrix cores), three classes, a minibatch of
# 256: the reference does not rescale a minibatch's likelihood to the dataset (variables.py:849), so the entropy term of every weight
# is weighed against 256 rows only, and a wider input or a smaller minibatch lets the posterior's noise drown the data
KW = dict(batch_size=256, n_features=64, n_hidden=20, n_classes=3, q_scale=0.05, q_scale1=0.02, pixels="integers", teacher=5)


def data_of(model):
    """(pixels [DS, P], labels [DS]) behind the model's two EmpiricalVariables"""
    by_name = {v.name: v for v in model.flatten()}
    array = lambda v: np.asarray(v.link.expressions()["dataset"].expr.attr.value)
    return array(by_name["x"]).astype(np.float32).reshape(-1, KW["n_features"]), array(by_name["k"].dataset).reshape(-1).astype(np.int64)


def accuracy(compiled, pixels, labels, samples=64):
    mean = compiled.predict(pixels, samples)["mean"]                       # [rows, classes], on the device
    return float((mean.argmax(1).cpu().numpy() == labels).mean())


model = W.build_bayesian_neural_network(W.native_api(), dataset_size=4096, seed=0, **KW)
held_out = data_of(W.build_bayesian_neural_network(W.native_api(), dataset_size=2000, seed=1, **KW))
train_set = data_of(model)
compiled = engine.compile_model(model)
print("engine: %s, training data path %s, predict kernel in %s" % (type(compiled).__name__, compiled.data_path(), compiled.predict_path()))
print("accuracy before training: held out %.3f, training rows %.3f (%d classes)" % (accuracy(compiled, *held_out), accuracy(compiled, *train_set), KW["n_classes"]))
t0 = time.time()
inference.perform_inference(model, number_iterations=ITERATIONS, number_samples=50, optimizer="Adam", lr=LR)
seconds = time.time() - t0
loss = np.asarray(model.diagnostics["loss curve"])
print("%d iterations in %.2f s; loss %.1f -> %.1f" % (ITERATIONS, seconds, loss[:20].mean(), loss[-20:].mean()))
torch.cuda.synchronize()
t0 = time.time()
acc = accuracy(compiled, *held_out)
torch.cuda.synchronize()
print("accuracy after training:  held out %.3f (2 000 rows x 64 weight samples in %.1f ms), training rows %.3f" % (
    acc, (time.time() - t0) * 1e3, accuracy(compiled, *train_set)))
# the reference's own call, one held-out row at a time as its script does
x = next(v for v in model.flatten() if v.name == "x")
k = next(v for v in model.flatten() if v.name == "k")
hits = 0
for row, label in zip(held_out[0][:20], held_out[1][:20]):
    sample = model._get_posterior_sample(10, input_values={x: torch.from_numpy(row.reshape(1, 1, -1, 1))})[k]      # one-hot [10, 1, classes, 1]
    hits += int(sample.cpu().numpy().mean(axis=0).reshape(-1).argmax() == label)
print("model._get_posterior_sample(10, input_values={x: row})[k], 20 held-out rows: %d right" % hits)
